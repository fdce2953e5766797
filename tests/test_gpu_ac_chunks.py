"""Chunk-parallel range coder on the GPU (include/scp.h, "Chunk-parallel range coder"): scp_ac_chunks_encode_lohi writes, chunk by chunk,
the bytes the host coder (native.ac_encode_lohi) writes for the slice, and scp_ac_chunks_decode_ctx returns, chunk by chunk, the symbols
the host decoder (AcDecoder.run_ctx) returns on the chunk's bytes - whole or cut short.  Every expected value comes from the host coder
on slices; none from the code under test.  The pair sets and their host-coded chunks are built once per process."""
import numpy as np
import pytest
import torch

from chunk_cases import CHUNKS, KINDS, host_chunks, lohi_of, pairs, sizes, table_symbols
from test_gpu_ringrate import dev

pytestmark = pytest.mark.gpu

ALPHABETS = (511, 1021)
GUARD, PATTERN = 4096, 0xA5


@pytest.fixture(scope="module", autouse=True)
def leave_the_process_as_found():
    yield
    import gc
    pairs.cache_clear()
    host_chunks.cache_clear()
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


@pytest.mark.parametrize("N", CHUNKS)
@pytest.mark.parametrize("kind", KINDS)
def test_encoder_writes_the_host_coders_bytes_chunk_by_chunk(kind, N):
    from scp_amd import native
    for n in sizes(N):
        want = host_chunks(kind, n, N)
        lengths, data = native.ac_chunks_encode(torch.from_numpy(pairs(kind, n).view(np.int32).copy()).to(dev()), N)
        assert lengths.dtype == np.uint32 and lengths.tolist() == [len(c) for c in want], (kind, N, n)
        assert data == b"".join(want), (kind, N, n)


def raw_encode(lohi, N, cap, guard=GUARD):
    """The C entry with a caller-made `out` of cap bytes inside a guard region -> (rc, status, lengths, the whole buffer)."""
    from scp_amd import native
    L = native.lib()
    n = len(lohi)
    C = -(-n // N)
    d = torch.from_numpy(lohi.view(np.int32).copy()).to(dev())
    nb = L.scp_ac_chunks_workspace_bytes(n, N)
    ws = torch.empty(nb // 8 + 1, dtype=torch.int64, device=dev())
    out = torch.full((guard + cap + guard,), PATTERN, dtype=torch.uint8, device=dev())
    lengths = torch.full((C + 2,), -1, dtype=torch.int32, device=dev())
    status = torch.full((1,), 77, dtype=torch.int32, device=dev())
    rc = L.scp_ac_chunks_encode_lohi(d.data_ptr(), n, N, lengths.data_ptr(), out.data_ptr() + guard, cap, status.data_ptr(), ws.data_ptr(), nb,
                                     torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, int(status.item()), lengths.cpu().numpy(), out.cpu().numpy()


def test_a_small_cap_is_reported_and_nothing_behind_it_is_touched():
    from scp_amd import native
    N, n = 64, 64 * 64 + 1
    p = pairs("tab1021", n)
    want = host_chunks("tab1021", n, N)
    total = sum(len(c) for c in want)
    rc, status, lengths, buf = raw_encode(p, N, total)                 # exactly enough
    assert (rc, status) == (0, 0) and lengths[:len(want)].tolist() == [len(c) for c in want] and lengths[len(want):].tolist() == [-1, -1]
    assert buf[GUARD:GUARD + total].tobytes() == b"".join(want)
    assert (buf[:GUARD] == PATTERN).all() and (buf[GUARD + total:] == PATTERN).all()
    for cap in (total - 1, total // 2 // 4 * 4, 0):
        rc, status, lengths, buf = raw_encode(p, N, cap)
        assert rc == 0 and status == -3                                # SCP_ESMALL through status, as the host coder returns it
        assert lengths[:len(want)].tolist() == [len(c) for c in want]  # the lengths are complete: the caller can size the next call
        assert (buf[GUARD + cap:] == PATTERN).all() and (buf[:GUARD] == PATTERN).all()
    with pytest.raises(native.ScpError, match="SCP_ESMALL"):
        native.ac_chunks_encode(torch.from_numpy(p.view(np.int32).copy()).to(dev()), N, cap=total - 1)


def test_argument_errors_return_einval_and_launch_nothing():
    from scp_amd import native
    L = native.lib()
    assert L.scp_ac_chunks_workspace_bytes(-1, 4096) == -1 and L.scp_ac_chunks_workspace_bytes(100, -4096) == -1
    assert L.scp_ac_chunks_workspace_bytes(100, 63) == -1 and L.scp_ac_chunks_workspace_bytes(100, (1 << 20) + 1) == -1
    assert L.scp_ac_chunks_workspace_bytes(0, 64) == 8
    assert L.scp_ac_chunks_workspace_bytes(129, 64) == 4 * 8 + 3 * 4 * ((18 * 64 + 2 + 31) // 32)
    z = torch.zeros(64, dtype=torch.int64, device=dev())
    p, st = z.data_ptr(), torch.cuda.current_stream().cuda_stream
    nb = L.scp_ac_chunks_workspace_bytes(64, 64)
    assert nb <= 64 * 8 - 64
    enc = lambda n=64, N=64, cap=64, status=p, ws=p, nbytes=nb, out=p + 256: L.scp_ac_chunks_encode_lohi(p, n, N, p + 128, out, cap, status, ws, nbytes, st)
    assert enc(n=-1) == enc(N=63) == enc(N=(1 << 20) + 1) == enc(cap=-1) == enc(status=None) == enc(ws=None) == enc(nbytes=nb - 1) == -1
    assert enc(ws=p + 4) == enc(out=p + 257) == -1
    dec = lambda n=8, N=64, ntab=1, Lp=8, nctx=1, off=p, tabs=p + 64: L.scp_ac_chunks_decode_ctx(p + 128, off, n, N, tabs, ntab, Lp, p + 192, nctx, p + 200, p + 256, st)
    assert dec(n=-1) == dec(N=63) == dec(ntab=0) == dec(ntab=257) == dec(Lp=1) == dec(nctx=0) == dec(nctx=257) == dec(off=None) == dec(tabs=None) == -1
    assert dec(ntab=16, Lp=4096) == -1                                 # 128 KB of tables do not fit into LDS
    torch.cuda.synchronize()
    assert not z.any()
    c = torch.zeros(8, dtype=torch.uint8, device=dev())
    for bad, why in ((dict(N=63), "64 .. 2\\^20"), (dict(lengths=[1, 1]), "1 expected"), (dict(lengths=[3]), "add up"), (dict(table_of=[1]), "table index"),
                     (dict(ctx=c + 1), "context 1 of 1")):
        a = dict(dict(payload=b"\0\0", lengths=[2], N=64, tables=np.zeros((1, 8), np.uint16), table_of=[0], ctx=c), **bad)
        with pytest.raises(native.ScpError, match=why):
            native.ac_chunks_decode(a["payload"], a["lengths"], a["N"], a["tables"], a["table_of"], a["ctx"], 8)


def host_decode(chunk, tabs, table_of, ctx, Lp):
    from scp_amd import native
    return native.AcDecoder(chunk, Lp=Lp).run_ctx(tabs[np.asarray(table_of)], ctx)


@pytest.mark.parametrize("alphabet", ALPHABETS)
@pytest.mark.parametrize("N", (64, 256))
def test_decoder_returns_the_source_symbols_and_the_host_decoders_on_cut_chunks(alphabet, N):
    """Host-coded and device-coded chunks decode to the source symbols through a context -> table map with fewer tables than contexts;
    chunks cut by 1 .. 4 bytes (the length table cut with them) decode to what the host decoder returns on the cut bytes; `sym` sits in
    a guard region."""
    from scp_amd import native
    rng = np.random.default_rng(alphabet + N)
    Lp = alphabet + 1
    for n in (1, N + 1, 65 * N - 1):
        tabs, tctx, sym = table_symbols(rng, n, alphabet)
        nctx = 40                                                      # 40 contexts on 16 tables: the map is not the identity
        table_of = rng.integers(0, 16, size=nctx)
        ctx = np.array([rng.choice(np.nonzero(table_of == g)[0]) if (table_of == g).any() else 0 for g in tctx], np.uint8)
        lohi = lohi_of(tabs, table_of[ctx].astype(np.uint8), sym)
        chunks = [native.ac_encode_lohi(lohi[b:b + N]) for b in range(0, n, N)]
        d_ctx = torch.from_numpy(ctx).to(dev())
        got = native.ac_chunks_decode(b"".join(chunks), [len(c) for c in chunks], N, tabs, table_of, d_ctx, Lp)
        assert got.dtype == torch.int16 and got.cpu().numpy().tolist() == sym.tolist()
        lengths, data = native.ac_chunks_encode(torch.from_numpy(lohi.view(np.int32).copy()).to(dev()), N)
        assert data == b"".join(chunks)
        assert torch.equal(native.ac_chunks_decode(data, lengths, N, tabs, table_of, d_ctx, Lp), got)
        cuts = [min(len(c), 1 + (i % 4)) for i, c in enumerate(chunks)]
        short = [c[:len(c) - k] for c, k in zip(chunks, cuts)]
        want = np.concatenate([host_decode(c, tabs, table_of, ctx[i * N:(i + 1) * N], Lp) for i, c in enumerate(short)])
        # through the C entry, `sym` inside a guard region
        L = native.lib()
        off = np.zeros(len(short) + 1, np.int64)
        np.cumsum([len(c) for c in short], out=off[1:])
        d_bytes = torch.from_numpy(np.frombuffer(b"".join(short) + b"\xff" * 8, np.uint8).copy()).to(dev())      # (ones behind the last chunk: zero fill must not read them)
        d_off, d_tab = torch.from_numpy(off).to(dev()), torch.from_numpy(tabs.view(np.int16).copy()).to(dev())
        d_map = torch.from_numpy(table_of.astype(np.uint8)).to(dev())
        out = torch.full((GUARD + n + GUARD,), 0x5A5A, dtype=torch.int16, device=dev())
        rc = L.scp_ac_chunks_decode_ctx(d_bytes.data_ptr(), d_off.data_ptr(), n, N, d_tab.data_ptr(), 16, Lp, d_map.data_ptr(), nctx, d_ctx.data_ptr(),
                                        out.data_ptr() + 2 * GUARD, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        o = out.cpu().numpy()
        assert rc == 0 and o[GUARD:GUARD + n].tolist() == want.tolist()
        assert (o[:GUARD] == 0x5A5A).all() and (o[GUARD + n:] == 0x5A5A).all()
        assert native.ac_chunks_decode(b"".join(short), [len(c) for c in short], N, tabs, table_of, d_ctx, Lp).cpu().numpy().tolist() == want.tolist()


def test_out_of_range_contexts_and_table_indices_read_inside_the_tables():
    """The wrapper refuses them; the kernel clamps them, so a caller of the C entry that skips the check reads no table out of range."""
    from scp_amd import native
    L = native.lib()
    n, N, Lp = 200, 64, 512
    tabs = np.ascontiguousarray(native_tables(511)[:2])
    ctx = torch.full((n,), 255, dtype=torch.uint8, device=dev())
    d_map = torch.tensor([0, 200, 1], dtype=torch.uint8, device=dev())
    d_tab = torch.from_numpy(tabs.view(np.int16).copy()).to(dev())
    chunk = bytes(range(40))
    d_bytes = torch.from_numpy(np.frombuffer(chunk * 4, np.uint8).copy()).to(dev())
    d_off = torch.tensor([0, 40, 80, 120, 160], dtype=torch.int64, device=dev())
    out = torch.zeros(n, dtype=torch.int16, device=dev())
    rc = L.scp_ac_chunks_decode_ctx(d_bytes.data_ptr(), d_off.data_ptr(), n, N, d_tab.data_ptr(), 2, Lp, d_map.data_ptr(), 3, ctx.data_ptr(), out.data_ptr(),
                                    torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    want = np.concatenate([native.AcDecoder(chunk, Lp=Lp).run_ctx(tabs[1:2], np.zeros(min(N, n - b), np.uint8)) for b in range(0, n, N)])
    assert rc == 0 and out.cpu().numpy().tolist() == want.tolist()          # context 255 -> 2, table_of[2] = 1


def native_tables(alphabet):
    from scp_amd import attr
    return attr.tables(alphabet)
