"""The lockstep EHEM decoder's host side (no GPU): the schedule against the one-stream decoder's loop, the round layout and its cut
into phase-1 runs, the slice property of the packed plan that phase 2 of a step relies on, and the CLI flag."""
import numpy as np
import pytest
import torch

# made-up files: a list of trees, each a list of level sizes (level 1 = the root); `drop`: the last node of every tree's last level
# is not coded (a multi-level frame)
_FILES = [
    ([[1, 3, 9, 20, 31], [1, 2, 5, 11, 23, 30], [1, 4, 9, 17, 29, 41, 57]], True),       # multi-level, last levels drop a node
    ([[1, 8, 23, 50]], False),
    ([[1, 1, 1], [1, 1, 1, 1], [1, 1, 1, 1, 1]], True),                                  # one-leaf shells: the last level is the dropped node alone
    ([[1]], False),                                                                      # a one-node frame
    ([[1, 5, 8, 8, 15, 29, 36, 64]], False),
    ([[1], [1, 2], [1, 2, 3]], True),                                                    # a shell that is its dropped root
    ([[1, 7, 7, 28]], False),
]


def _one_stream(trees, drop, cs):
    """The (tree, level, window, length) sequence of FrameDecoder._decode_tree (levels) and decoder.window_lengths (windows) for one file."""
    out = []
    for t, sizes in enumerate(trees):
        depth = len(sizes)
        for L in range(1, depth + 1):
            n = sizes[L - 1]
            rows = n - (1 if (drop and L == depth) else 0)
            if rows > 0:
                for k, i in enumerate(range(0, rows, cs)):
                    out.append((t, L, k, min(cs, rows - i)))
    return out


def _drive(files, slots, cs):
    """EhemLockstep over `files` -> (per file its (tree, level, window, length) sequence, the refills [(round, slot, file)], the slots
    ever active)."""
    from scp_amd.decoder import EhemLockstep
    sched = EhemLockstep([[len(t) for t in trees] for trees, _ in files], [d for _, d in files], slots, cs)
    seq = [[] for _ in files]
    refills = [(0, s, f) for s, f in sched.refill()]
    used, rnd = set(), 0
    while True:
        info = sched.round()
        if not info:
            break
        assert [r[0] for r in info] == list(sched.active()) == sorted(r[0] for r in info)
        rows = []
        for s, f, t, L, n, r in info:
            trees, drop = files[f]
            assert n == trees[t][L - 1] and r == n - (1 if drop and L == len(trees[t]) else 0), (s, f, t, L)
            rows.append(r)
            used.add(s)
        steps, wbase = EhemLockstep.layout(rows, cs)
        nwin = [-(-r // cs) for r in rows]
        assert len(steps) == max(nwin)
        for k, step in enumerate(steps):
            assert [c for c, _ in step] == [c for c, w in enumerate(nwin) if w > k], "step k holds exactly the slots with more than k windows"
            for col, c in step:
                s, f, t, L, _, _ = info[col]
                seq[f].append((t, L, k, c))
        rnd += 1
        for s, f, t, L, n, _ in info:
            trees = files[f][0]
            last = L == len(trees[t])
            st = sched.advance(s, 3 if last else trees[t][L])
            assert st == ("level" if not last else "tree" if t + 1 < len(trees) else "file")
        refills += [(rnd, s, f) for s, f in sched.refill()]
    assert not sched.pending
    return seq, refills, used


@pytest.mark.parametrize("cs", [4, 7])
@pytest.mark.parametrize("slots", [1, 2, 3, 5])
def test_schedule_equals_the_one_stream_loop(slots, cs):
    seq, refills, used = _drive(_FILES, slots, cs)
    for f, (trees, drop) in enumerate(_FILES):
        want = _one_stream(trees, drop, cs)
        assert seq[f] == want, f
    assert any(len(w) > 1 for w in ([c for *_, c in s] for s in seq)) and max(k for s in seq for _, _, k, _ in s) >= 3
    # refill order, simulated independently: a file occupies its slot for one round per level of all its trees; idle slots take the
    # pending files in file order, lowest slot first
    free_at, nxt, want = [0] * slots, 0, []
    rnd = 0
    while nxt < len(_FILES):
        for s in range(slots):
            if free_at[s] <= rnd and nxt < len(_FILES):
                want.append((rnd, s, nxt))
                free_at[s] = rnd + sum(len(t) for t in _FILES[nxt][0])
                nxt += 1
        rnd = min(free_at)
    assert refills == want
    assert used == set(range(min(slots, len(_FILES))))


def test_more_slots_than_files_leaves_slots_idle():
    seq, refills, used = _drive(_FILES[:3], 5, 4)
    assert used == {0, 1, 2} and refills == [(0, 0, 0), (0, 1, 1), (0, 2, 2)]
    for f in range(3):
        assert seq[f] == _one_stream(*_FILES[f], 4)


@pytest.mark.parametrize("rows,cs", [([700, 1, 1030, 5, 2, 8192, 33], 512), ([0, 9, 0, 1], 4), ([5], 7), ([0, 0], 3), ([16384, 8193, 3], 8192)])
def test_round_layout_is_dense_and_step_major(rows, cs):
    from scp_amd.decoder import EhemLockstep, window_lengths
    steps, wbase = EhemLockstep.layout(rows, cs)
    T = sum(rows)
    seen = np.zeros(T, np.int64)
    row = 0
    for k, step in enumerate(steps):
        assert [c for c, _ in step] == sorted(c for c, _ in step)
        for col, c in step:
            assert wbase[k, col] == row, "the windows of a step are adjacent, in slot order"
            assert c == window_lengths(rows[col], cs)[k]
            seen[row:row + c] += 1
            row += c
    assert row == T and (seen == 1).all()
    assert wbase.shape == (max([-(-r // cs) for r in rows] + [1]), len(rows))
    for col, r in enumerate(rows):
        assert (wbase[-(-r // cs):, col] == -1).all() and (wbase[:-(-r // cs), col] >= 0).all()


def test_chunk_cutter_keeps_steps_whole_under_both_bounds():
    from scp_amd.decoder import EhemLockstep, chunk_steps
    from scp_amd.encoder import MAX_PACKED_ROWS
    pad = lambda st: sum(-(-(c + (c & 1)) // 512) * 512 for c in st)
    # more than 1 000 000 tokens: 40 slots of 5 full windows and a tail
    steps, _ = EhemLockstep.layout([5 * 8192 + 17 * (s % 3) for s in range(40)], 8192)
    lens = [[c for _, c in st] for st in steps]
    cuts = chunk_steps(lens)
    assert len(cuts) >= 2 and sum(map(sum, lens)) > 1_000_000
    # more than MAX_PACKED_ROWS padded rows with few tokens: 64 slots of 40 one-node windows
    steps2, _ = EhemLockstep.layout([40] * 64, 1)
    lens2 = [[c for _, c in st] for st in steps2]
    cuts2 = chunk_steps(lens2)
    assert len(cuts2) >= 2 and sum(map(pad, lens2)) > MAX_PACKED_ROWS and sum(map(sum, lens2)) < 1_000_000
    for ln, ct in ((lens, cuts), (lens2, cuts2)):
        assert ct[0][0] == 0 and ct[-1][1] == len(ln) and all(a[1] == b[0] for a, b in zip(ct, ct[1:]))
        for i, j in ct:
            assert j > i
            assert sum(map(sum, ln[i:j])) <= 1_000_000 and sum(map(pad, ln[i:j])) <= MAX_PACKED_ROWS
            if j < len(ln):          # greedy: the next step would not have fitted
                assert sum(map(sum, ln[i:j + 1])) > 1_000_000 or sum(map(pad, ln[i:j + 1])) > MAX_PACKED_ROWS
    # one step of 64 slots x 8192 tokens fits both bounds; a step that exceeds a bound goes alone, whole
    assert chunk_steps([[8192] * 64]) == [(0, 1)] and 64 * 8192 <= min(1_000_000, MAX_PACKED_ROWS)
    assert chunk_steps([[8], [9, 9], [3]], max_tokens=10) == [(0, 1), (1, 2), (2, 3)]
    assert chunk_steps([]) == []


_WINDOWS = [700, 1, 1030, 5, 2, 8192, 33, 511, 512, 513, 7]
_GROUPS = [(2, 5), (1, 2), (5, 7), (7, 10), (0, 1), (10, 11), (0, 11), (3, 8)]


@pytest.fixture(scope="module")
def full_plan():
    from scp_amd.models.packed import PackedPlan
    return PackedPlan(_WINDOWS, device="cpu", use_native=False)


@pytest.mark.parametrize("i,j", _GROUPS, ids=[str(_WINDOWS[i:j]) for i, j in _GROUPS])
def test_a_group_of_adjacent_windows_is_a_slice_of_the_longer_plan(full_plan, i, j):
    """Windows i .. j - 1 of a plan occupy, in every self and cross stage, one contiguous run of rows, and every map of the plan restricted
    to that run equals the group's own plan relative to the run's first row: what phase 2 of a step computes on its slice of the
    round-wide phase-1 state and preparation is what the group's own forward computes."""
    from scp_amd.models.packed import PackedPlan
    F, G = full_plan, PackedPlan(_WINDOWS[i:j], device="cpu", use_native=False)
    tok0 = sum(_WINDOWS[:i])
    for kind in ("self", "cross"):
        fl, gl = getattr(F, kind + "_layouts"), getattr(G, kind + "_layouts")
        base = [int(l.base[i]) for l in fl]
        for s, (a, b) in enumerate(zip(fl, gl)):
            assert torch.equal(a.Lp[i:j], b.Lp) and torch.equal(a.base[i:j] - base[s], b.base)          # contiguous, same padding
            assert base[s] % 512 == 0
            lo, hi = base[s], base[s] + b.rows
            assert torch.equal(F.d[kind + "_valid"][s][lo:hi], G.d[kind + "_valid"][s])
            ft = F.d[kind + "_tab"][s][lo // 512:hi // 512].clone()
            ft[:, 0] -= lo
            assert torch.equal(ft, G.d[kind + "_tab"][s])
        for s in range(len(fl) - 1):
            lo, hi = base[s + 1], base[s + 1] + gl[s + 1].rows
            for fm, gm in zip(F.d[kind + "_merge"][s], G.d[kind + "_merge"][s]):
                f = fm[lo:hi]
                rel = torch.where(f == fl[s].rows, torch.full_like(f, gl[s].rows), f - base[s])         # the zero row of either plan
                assert torch.equal(rel, gm)
            lo, hi = base[s], base[s] + gl[s].rows
            real = G.d[kind + "_valid"][s].reshape(-1) > 0
            fp, gp = F.d[kind + "_parent"][s][lo:hi], G.d[kind + "_parent"][s]
            assert torch.equal((fp - base[s + 1])[real], gp[real]) and bool((gp[~real] == 0).all())
        for s in range(1, len(fl)):
            lo, hi = base[0], base[0] + gl[0].rows
            real = G.d[kind + "_valid"][0].reshape(-1) > 0
            fc, gc = F.d[kind + "_concat"][s - 1][lo:hi], G.d[kind + "_concat"][s - 1]
            assert torch.equal((fc - base[s])[real], gc[real])
    p0, q0 = int(F.self_layouts[0].base[i]), int(F.cross_layouts[0].base[i])
    Q, P = G.cross_layouts[0].rows, G.self_layouts[0].rows
    real = G.d["cross_valid"][0].reshape(-1) > 0
    for name in ("a1map", "a2map"):
        assert torch.equal((F.d[name][q0:q0 + Q] - p0)[real], G.d[name][real])
    fin = F.d["inmap"][p0:p0 + P]
    assert torch.equal(torch.where(fin == F.n_tokens, torch.full_like(fin, G.n_tokens), fin - tok0), G.d["inmap"])
    knn = F.d["knn_tab"][p0 // 512:(p0 + P) // 512].clone()
    knn[:, 0] -= p0
    assert torch.equal(knn, G.d["knn_tab"])
    for name in ("even_out", "odd_out"):
        f = F.d[name][q0:q0 + Q]
        assert torch.equal(torch.where(f < 0, f, f - tok0), G.d[name])
    c = torch.tensor(_WINDOWS)
    e0, o0 = int(((c[:i] + 1) // 2).sum()), int((c[:i] // 2).sum())
    ne, no = int(((c[i:j] + 1) // 2).sum()), int((c[i:j] // 2).sum())
    assert torch.equal(F.d["even_rows"][e0:e0 + ne] - q0, G.d["even_rows"]) and torch.equal(F.d["odd_rows"][o0:o0 + no] - q0, G.d["odd_rows"])
    assert torch.equal(F.d["even_dst"][e0:e0 + ne] - tok0, G.d["even_dst"]) and torch.equal(F.d["odd_dst"][o0:o0 + no] - tok0, G.d["odd_dst"])


def test_stage_rows_of_a_window_equal_the_plans():
    from scp_amd.decoder import _stage_rows
    from scp_amd.models.packed import PackedPlan
    for c in (1, 2, 5, 511, 1023, 1024, 1025, 1030, 8192):
        p = PackedPlan([c], device="cpu", use_native=False)
        assert _stage_rows(c, 4) == [l.rows for l in p.cross_layouts], c


@pytest.mark.parametrize("mullevel", [False, True])
def test_cli_streams_flag(mullevel, capsys):
    from scp_amd import cli
    assert cli.get_decode_args([]).streams == 1 and cli.get_decode_args(["--streams", "64"]).streams == 64
    for bad in ("0", "65"):
        with pytest.raises(SystemExit):
            cli.decode_main(["--streams", bad, "--random_weights", "0"], mullevel=mullevel)
        assert "--streams" in capsys.readouterr().err


def test_decode_files_refuses_a_bad_stream_count():
    from scp_amd import native
    from scp_amd.decoder import decode_files
    for s in (0, 65):
        with pytest.raises(native.ScpError, match="streams"):
            decode_files([], None, streams=s)
    assert decode_files([], None, streams=3) == []

