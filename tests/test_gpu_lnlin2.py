"""The two forms of the LayerNorm + projection kernel - rc_ln_linear_kernel (csrc/rowchain.hip, one workgroup per CU) and ln2_proj_kernel
(csrc/lnlin2.hip, two per CU) - give the same bits.  Which one a launch runs is decided by SCP_LNLIN, read once per process, so each setting
gets a fresh child process of its own (this file run as a script); a child writes one SHA-256 per output tensor - computed over every byte
of it on the host - and the test compares the two lists."""
import hashlib
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

QKV_M = (128, 256, 128 * 257, 590848)
PLAIN_M = (1, 127, 129) + QKV_M
CHILD_TIMEOUT = 900


def _valid(torch, M, g):
    """zeroes whole 128-row tiles (the second, where there is one, and the last), single rows and a random tenth"""
    v = (torch.rand(M, generator=g) > 0.1).float()
    if M >= 256:
        v[128:256] = 0
    if M >= 1024:
        v[M - 128:] = 0
    v[0] = 1
    v[min(5, M - 1)] = 0
    v[M - 1] = 0 if M > 1 else 1
    return v


def _sha(torch, t):
    return hashlib.sha256(t.detach().cpu().contiguous().view(torch.uint8).numpy()).hexdigest()


def _child(path):
    import torch
    sys.path.insert(0, ROOT)
    from scp_amd import native
    native.lib()
    dev = torch.device("cuda:0")
    g = torch.Generator(device="cpu").manual_seed(20)
    gamma = (1 + 0.1 * torch.randn(256, generator=g)).to(dev)
    beta = (0.1 * torch.randn(256, generator=g)).to(dev)
    fws, biases = {}, {}
    for N in (256, 512, 768):
        W = (torch.randn((N, 256), generator=g) * 0.05).to(dev)
        fws[N] = native.LnFoldedWeight(W, gamma, beta)
        biases[N] = (torch.randn(N, generator=g) * 0.1).to(dev)
    out = {}
    for M in PLAIN_M:
        x = (torch.randn((M, 256), generator=g) * 1.5 + 0.3).to(dev)
        valid = _valid(torch, M, g).to(dev)
        for use_valid in (False, True):
            v = valid if use_valid else None
            for N in (256, 512, 768):
                o = native.swin_ln_linear(x, fws[N], biases[N], 1e-5, v)
                torch.cuda.synchronize()
                out[f"plain M={M} N={N} valid={int(use_valid)}"] = _sha(torch, o)
                del o
                if M in QKV_M and N != 256:
                    q, kv = native.swin_ln_qkv(x, fws[N], biases[N], 1e-5, v)
                    torch.cuda.synchronize()
                    key = f"qkv M={M} N={N} valid={int(use_valid)}"
                    if N == 768:
                        out[key + " q"] = _sha(torch, q)
                    for p, name in enumerate(("K hi", "K lo", "Vt hi", "Vt lo")):
                        out[key + " " + name] = _sha(torch, kv.t[p])
                    del q, kv
        # a projection without bias (W beta alone) on the ragged sizes
        if M < 128 or M == 129:
            o = native.swin_ln_linear(x, fws[256], None, 1e-5, None)
            torch.cuda.synchronize()
            out[f"plain M={M} N=256 nobias"] = _sha(torch, o)
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)


def _run_child(mode, path):
    env = dict(os.environ, SCP_LNLIN=str(mode))
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(path)], env=env, capture_output=True, text=True, timeout=CHILD_TIMEOUT)
    assert r.returncode == 0, (mode, r.stdout[-2000:], r.stderr[-2000:])
    return json.load(open(path))


@pytest.mark.gpu
def test_two_per_cu_form_gives_the_same_bits(tmp_path):
    old = _run_child(1, tmp_path / "old.json")
    new = _run_child(2, tmp_path / "new.json")
    assert len(old) == 2 * (3 * len(PLAIN_M) + 9 * len(QKV_M)) + 3, len(old)
    assert set(old) == set(new)
    bad = [k for k in sorted(old) if old[k] != new[k]]
    assert not bad, bad[:20]


if __name__ == "__main__":
    assert sys.argv[1] == "--child"
    _child(sys.argv[2])
