"""alacgpu_resample_rows_device and alacgpu_plan_crops_frames_device on the GPU.

The resampler with a table per row against its specification in numpy (resample.apply_table with the row's own table), element
by element, and against alacgpu_resample_device run on the row alone, bit for bit.  The tolerance of an output is that of
tests/test_resample.py with row r's own N_r = 2 * width_r + 1: (N_r + 2) * 2^-24 * sum_k |w_k x_k|, computed from the
specification -- the forward error bound of a chain of N_r float32 fused multiply-adds (N_r * u * sum |w x| to first order,
u = 2^-24), one u more for the final rounding and one for the mono add in front.  It is derived, not measured, and no element
is left out.

The planner with a window length per crop against corpus_plan_host(crop_frames=...): exact, nothing there has a tolerance."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GUARD = 64
CFG = [(4096, 16, 40, 10, 14, 2)]


def up(torch, x, dt):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(x, dtype=dt))).to("cuda")


class Tables:
    """The tables of sources of `rates` going to `target`, on the host and on the device"""

    def __init__(self, torch, rates, target):
        from alac.net_amd.resample import rows_tables

        self.table_of, self.desc, d0, w = rows_tables(rates, target)
        self.host = [(int(a), int(b), int(width), d0[i:i + b], w[j:j + b * (2 * width + 1)].reshape(b, -1)) for a, b, width, i, j in self.desc.tolist()]
        self.d_desc, self.d_d0, self.d_w = up(torch, self.desc.view(np.int32), np.int32), up(torch, d0, np.int32), up(torch, w, np.float32)
        self.device = [(self.d_d0[i:i + b], self.d_w[j:j + b * (2 * width + 1)]) for a, b, width, i, j in self.desc.tolist()]


def guarded(torch, n):
    raw = torch.full(((n + 2 * GUARD) * 4,), 0x5A, dtype=torch.uint8, device="cuda").view(torch.float32)
    return raw, raw[GUARD:GUARD + n]


def intact(torch, raw, n):
    return bool((torch.cat([raw[:GUARD], raw[GUARD + n:]]).view(torch.uint8) == 0x5A).all())


def run_rows(torch, ctx, tabs, src, origin, valid, first, out_frames, row_table, mono):
    """One call over src [rows, C, stride] (numpy float32) into an output with GUARD elements of 0x5A bytes on both sides;
    returns (out [rows, C or 1, out_frames] numpy, guards intact, the device inputs for a call of the one-table entry)"""
    rows, C_, stride = src.shape
    Co = 1 if mono else C_
    n = rows * Co * out_frames
    raw, out = guarded(torch, n)
    dev = (up(torch, src, np.float32), up(torch, origin, np.int64), up(torch, valid, np.int64), up(torch, first, np.int64))
    ctx.resample_rows_device(dev[0], rows, C_, stride, dev[1], dev[2], dev[3], out_frames, tabs.desc, tabs.d_desc, tabs.d_d0, tabs.d_w,
                             up(torch, np.asarray(row_table, dtype=np.uint32).view(np.int32), np.int32), mono, out,
                             stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return out.cpu().numpy().reshape(rows, Co, out_frames), intact(torch, raw, n), dev


def run_one(torch, ctx, tabs, t, dev, r, C_, stride, out_frames, mono):
    """alacgpu_resample_device on row r alone with table t"""
    Co = 1 if mono else C_
    a, b, width = tabs.host[t][:3]
    out = torch.empty((1, Co, out_frames), dtype=torch.float32, device="cuda")
    ctx.resample_device(dev[0][r:r + 1].contiguous(), 1, C_, stride, dev[1][r:r + 1].contiguous(), dev[2][r:r + 1].contiguous(),
                        dev[3][r:r + 1].contiguous(), out_frames, a, b, width, *tabs.device[t], mono, out,
                        stream=torch.cuda.current_stream().cuda_stream)
    return out.cpu().numpy()[0]


def row_shape(k, a, b, stride):
    """Row shape k of tests/test_resample.py's rows_for, (origin, valid, first): a whole signal, a later first frame, an origin
    the taps reach in front of, no signal, one frame, a signal shorter than its row, frames beyond 2^32, and a valid count
    above the stride and below zero"""
    origin = [0, 0, 5 * a + 3, 11, 7, 0, 10 ** 12, 0, 0]
    valid = [stride, stride, stride, 0, 1, stride // 3, stride, stride + 100, -5]
    first = [0, 3 * b + 1, ((5 * a + 3) * b) // a, 0, 0, 0, (10 ** 12 * b) // a - 5, 0, 0]
    return origin[k], valid[k], first[k]


def check_row(src_r, origin, valid, first, out_frames, table, mono, got_r, tag):
    from alac.net_amd.resample import apply_table

    N = 2 * table[2] + 1
    v = min(max(int(valid), 0), src_r.shape[-1])
    x = src_r[:, :v].astype(np.float64)
    kw = dict(mono=mono, origin=int(origin), first=int(first), num_frames=out_frames)
    want = apply_table(x, *table, **kw)
    tol = (N + 2) * 2.0 ** -24 * apply_table(x, *table, magnitude=True, **kw)
    err = np.abs(got_r.astype(np.float64) - want)
    print(f"{tag}: N {N}, max err {err.max():.3e}, max err / tol {np.max(err / np.maximum(tol, 1e-300)):.3f}, max |y| {np.abs(want).max():.3e}")
    assert np.isfinite(got_r).all(), tag
    assert (err <= tol).all(), (tag, int(np.argmax(err - tol)), float(err.max()))
    return want


def test_rows_with_three_tables_equal_their_specification_and_the_one_table_call():
    import torch

    import alac.net_amd as pkg

    rng = np.random.default_rng(16)
    stride, out_frames = 5000, 1500          # a tile of 1024 output frames and a partial one
    with pkg.AlacGpuContext(CFG) as ctx:
        tabs = Tables(torch, [44100, 48000, 16000], 16000)       # 441 : 160, 3 : 1 and the table that copies
        n_tables = len(tabs.host)
        assert n_tables == 3 and tabs.host[2][:3] == (1, 1, 1)
        for turn, (channels, mono) in enumerate(((1, False), (2, False), (2, True), (1, True))):
            # twelve rows cycle through the tables (another table first every turn) and the nine shapes; two rows without a table
            row_table = [(r + turn) % 3 for r in range(12)] + [n_tables, 0xFFFFFFFF]
            rows = len(row_table)
            src = rng.standard_normal((rows, channels, stride)).astype(np.float32)
            origin, valid, first = np.zeros(rows, np.int64), np.full(rows, stride, np.int64), np.zeros(rows, np.int64)
            for r in range(12):
                a, b = tabs.host[row_table[r]][:2]
                origin[r], valid[r], first[r] = row_shape(r % 9, a, b, stride)
                if 0 <= valid[r] < stride:           # what lies behind a row's signal must not matter
                    src[r, :, valid[r]:] = np.nan if r % 2 else 1e30
                if valid[r] < 0:
                    src[r] = np.nan
            got, whole, dev = run_rows(torch, ctx, tabs, src, origin, valid, first, out_frames, row_table, mono)
            assert whole, "a store outside d_out"
            assert got.shape == (rows, 1 if mono else channels, out_frames)
            for r in range(12):
                t = row_table[r]
                tag = f"C{channels} mono{int(mono)} row {r} table {t} shape {r % 9}"
                want = check_row(src[r], origin[r], valid[r], first[r], out_frames, tabs.host[t], mono, got[r], tag)
                if r % 9 in (3, 8):
                    assert not got[r].any(), tag                    # no signal: zeros, whatever the memory holds
                if r % 9 == 0:
                    assert got[r].any() and want.any(), tag
                if t == 2:
                    assert np.array_equal(got[r].astype(np.float64), want), tag     # the table that copies: exact
                alone = run_one(torch, ctx, tabs, t, dev, r, channels, stride, out_frames, mono)
                assert np.array_equal(got[r].view(np.uint32), alone.view(np.uint32)), tag      # bit for bit
            assert not got[12].any() and not got[13].any()          # a row without a table is zeros


def test_a_table_past_64_kib_of_lds_next_to_a_small_one():
    import torch

    import alac.net_amd as pkg

    rng = np.random.default_rng(17)
    with pkg.AlacGpuContext(CFG) as ctx:
        tabs = Tables(torch, [200000, 1000], 1000)                   # 200 : 1 and the table that copies
        a, b, width = tabs.host[0][:3]
        N = 2 * width + 1
        # at a tile of 256 output frames the 200 : 1 table and its span need more than 16384 floats: the launch takes more than
        # 64 KiB of LDS, and the rows of the small table share its tile
        assert b * N + (255 * a) // b + 2 * width + 2 > 16384
        out_frames = 300
        stride = out_frames * a - 77
        row_table = [0, 1, 0, 1, 0, 1]
        src = rng.standard_normal((6, 1, stride)).astype(np.float32)
        origin, valid, first = np.array([0, 0, 3, 10, 0, 0]), np.array([stride, stride, stride, 200, 5, 0]), np.array([0, 0, 1, 5, 0, 0])
        got, whole, dev = run_rows(torch, ctx, tabs, src, origin, valid, first, out_frames, row_table, False)
        assert whole, "a store outside d_out"
        for r, t in enumerate(row_table):
            check_row(src[r], origin[r], valid[r], first[r], out_frames, tabs.host[t], False, got[r], f"row {r} table {t}")
            alone = run_one(torch, ctx, tabs, t, dev, r, 1, stride, out_frames, False)
            assert np.array_equal(got[r].view(np.uint32), alone.view(np.uint32)), r
        assert np.array_equal(got[1, 0], src[1, 0, :out_frames]) and got[0].any() and not got[5].any()
        assert np.array_equal(got[3, 0, 5:205], src[3, 0, :200]) and not got[3, 0, :5].any() and not got[3, 0, 205:].any()


def test_bad_arguments_are_refused_before_anything_is_enqueued():
    import ctypes

    import torch

    import alac.net_amd as pkg

    L_ = pkg.lib()
    with pkg.AlacGpuContext(CFG) as ctx:
        t = torch.zeros(16384, dtype=torch.int64, device="cuda")      # (room for the largest table)
        p, q = pkg._dp(t), pkg._VP(t.data_ptr() + 4)
        desc = np.array([[2, 1, 13, 0, 0], [1, 1, 1, 0, 0]], dtype=np.uint32)
        d_desc = torch.from_numpy(desc.view(np.int32)).to("cuda")
        names = ["ctx", "src", "rows", "channels", "stride", "origin", "valid", "first", "out_frames", "tables", "d_tables", "n_tables",
                 "d0", "w", "row_table", "mono", "out", "stream"]
        good = dict(ctx=ctx._ctx, src=p, rows=1, channels=1, stride=64, origin=p, valid=p, first=p, out_frames=16, tables=pkg._ptr(desc),
                    d_tables=pkg._dp(d_desc), n_tables=2, d0=p, w=p, row_table=p, mono=0, out=p, stream=None)
        call = lambda **kw: L_.alacgpu_resample_rows_device(*[{**good, **kw}[k] for k in names])
        assert call() == 0 and call(mono=1) == 0 and call(channels=2, mono=1) == 0
        assert call(rows=0) == 0 and call(out_frames=0) == 0
        for k in ("ctx", "src", "origin", "valid", "first", "tables", "d_tables", "d0", "w", "row_table", "out"):
            assert call(**{k: None}) == -1, k
        for k in ("origin", "valid", "first"):
            assert call(**{k: q}) == -1, k                                                # 8-byte arrays at 4
        for k in ("src", "d_tables", "d0", "w", "row_table", "out", "origin"):
            assert call(**{k: pkg._VP(t.data_ptr() + 2)}) == -1, k
        assert call(n_tables=0) == -1 and call(channels=0) == -1 and call(channels=3) == -1
        # any table that would be refused alone, wherever it stands: no ratio, no width, more than 16384 weights
        for bad in ([0, 1, 13], [2, 0, 13], [2, 1, 0], [1, 160, 51], [1, 16385, 1], [1, 1, 8192]):
            for at in (0, 1):
                d = desc.copy()
                d[at, :3] = bad
                assert call(tables=d.ctypes.data_as(ctypes.c_void_p)) == -1, (bad, at)
        big = np.array([[1, 1, 8191, 0, 0]], dtype=np.uint32)                             # the largest table there is
        assert call(tables=pkg._ptr(big), d_tables=pkg._dp(torch.from_numpy(big.view(np.int32)).to("cuda")), n_tables=1, out_frames=2) == 0
        torch.cuda.synchronize()
        assert not t.any()                  # (zero weights over zeros: the calls that ran wrote zeros)


# ---- the planner with a window length per crop ---------------------------------------------------------------------------------
PLAN_GUARD = 16


def run_planner(torch, pkg, ctx, tb, crop_file, crop_offset, each, L, K, stride):
    """alacgpu_plan_crops_frames_device (each None: alacgpu_plan_crops_device) into arrays with guards of 0x5A bytes in front of
    and behind them; returns the seven arrays (device tensors, the unsigned types as their signed twins) and whether every
    guard is intact"""
    upv = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).view(dt) if len(a) else np.zeros(1, dt)).to("cuda")
    d_tab = [upv(tb["pkt_offset"], np.int64), upv(tb["pkt_size"], np.int32), upv(tb["pkt_end"], np.int64), upv(tb["file_first"], np.int32),
             upv(tb["file_cfg"], np.int16)]
    B = len(crop_file)
    d_cf, d_co = upv(np.asarray(crop_file, dtype=np.uint32), np.int32), upv(np.asarray(crop_offset, dtype=np.uint64), np.int64)
    kinds = [torch.int64, torch.int32, torch.int16, torch.int64, torch.int32, torch.int32, torch.int64]
    counts = [B * K] * 6 + [B]
    raw = [torch.full(((n + 2 * PLAN_GUARD) * torch.empty(0, dtype=k).element_size(),), 0x5A, dtype=torch.uint8, device="cuda").view(k)
           for n, k in zip(counts, kinds)]
    outs = [r[PLAN_GUARD:PLAN_GUARD + n] for r, n in zip(raw, counts)]
    front = [ctx._ctx, *[pkg._dp(t) for t in d_tab], len(tb["file_first"]) - 1, pkg._dp(d_cf), pkg._dp(d_co)]
    back = [B, L, K, stride, *[pkg._dp(t) for t in outs], pkg._VP(torch.cuda.current_stream().cuda_stream)]
    if each is None:
        rc = pkg.lib().alacgpu_plan_crops_device(*front, *back)
    else:
        d_each = upv(np.asarray(each, dtype=np.uint32), np.int32)
        rc = pkg.lib().alacgpu_plan_crops_frames_device(*front, pkg._dp(d_each), *back)
    assert rc == 0, rc
    torch.cuda.synchronize()
    whole = all(bool((torch.cat([r[:PLAN_GUARD], r[PLAN_GUARD + n:]]).view(torch.uint8) == 0x5A).all()) for r, n in zip(raw, counts))
    return outs, whole


def test_planner_with_a_length_per_crop_equals_its_host_twin():
    import torch

    import alac.net_amd as pkg
    from test_corpus_mixed_plan import tables_of

    rng = np.random.default_rng(18)
    # six files of 3 .. 40 packets: regular frames with a short last packet, 1024-frame packets, irregular ones with empty packets
    files = [[4096] * 2 + [100], [4096] * 39 + [4000], [1024] * 17 + [9], rng.choice([0, 1, 17, 1000, 4096], 25).tolist(), [4096] * 8,
             [1024] * 30 + [1]]
    tb = tables_of(files, rng)
    F, totals = len(files), [int(np.sum(d)) for d in files]
    bound, B = 20000, 64
    signed = {np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32, np.dtype(np.uint16): np.int16, np.dtype(np.int64): np.int64}
    names = ("offsets", "sizes", "cfg_idx", "dst_first", "dst_frames", "src_skip", "lengths")
    cf = rng.integers(0, F, B).astype(np.uint32)
    co = np.array([int(rng.integers(0, totals[f] + 1)) for f in cf], dtype=np.uint64)
    each = rng.integers(0, bound + 1, B).astype(np.uint32)
    each[:3] = (0, bound, 1)
    co[1] = 0
    each[7] = bound + 1                   # a length above the bound
    cf[9] = F                             # a file that does not exist
    co[11] = totals[int(cf[11])] + 1      # an offset past the end
    tabs = (tb["pkt_offset"], tb["pkt_size"], tb["pkt_end"], tb["file_first"], tb["file_cfg"])
    with pkg.AlacGpuContext(CFG) as ctx:
        K_all = max(pkg.entries_per_crop(tb["pkt_end"], tb["file_first"], bound), 1)
        for K in (K_all, 3):              # enough for every crop; too few for many (-2)
            stride = 2 * bound
            want = pkg.corpus_plan_host(*tabs, cf, co, bound, K, stride, crop_frames=each)
            got, whole = run_planner(torch, pkg, ctx, tb, cf, co, each, bound, K, stride)
            assert whole, f"a store outside the plan arrays (K {K})"
            for name, g, w in zip(names, got, want):
                w = torch.from_numpy(w.view(signed[w.dtype]))
                assert g.dtype == w.dtype and torch.equal(g.cpu(), w), (name, K, torch.nonzero(g.cpu() != w)[:5].tolist())
            assert want[6][[7, 9, 11]].tolist() == [-1, -1, -1] and want[6][0] == 0 and ((want[6] == -2).any() == (K == 3))
            assert (want[2].reshape(B, K)[7] == 0xFFFF).all()
            lens = want[6]
            fine = lens >= 0
            assert (lens[fine] == np.minimum(each[fine].astype(np.int64), np.array(totals)[cf[fine]] - co[fine].astype(np.int64))).all()
        # all lengths equal: the plan of the existing entry point, bit for bit
        for L in (4096, 12345):
            K = max(pkg.entries_per_crop(tb["pkt_end"], tb["file_first"], L), 1)
            a, whole_a = run_planner(torch, pkg, ctx, tb, cf, co, None, L, K, 2 * L)
            b, whole_b = run_planner(torch, pkg, ctx, tb, cf, co, np.full(B, L, np.uint32), L, K, 2 * L)
            assert whole_a and whole_b and all(torch.equal(x, y) for x, y in zip(a, b)), L
        # the argument checks: a no-op, a NULL and a misaligned array of lengths
        L_ = pkg.lib()
        t = torch.zeros(64, dtype=torch.int64, device="cuda")
        p = pkg._dp(t)
        args = lambda **kw: [ctx._ctx, p, p, p, p, p, 1, p, p, kw.get("each", p), kw.get("B", 1), 1, kw.get("K", 1), 0,
                             p, p, p, p, p, p, p, None]
        assert L_.alacgpu_plan_crops_frames_device(*args(B=0, K=0)) == 0
        assert L_.alacgpu_plan_crops_frames_device(*args()) == 0
        assert L_.alacgpu_plan_crops_frames_device(*args(K=0)) == -1
        assert L_.alacgpu_plan_crops_frames_device(*args(each=None)) == -1
        assert L_.alacgpu_plan_crops_frames_device(*args(each=pkg._VP(t.data_ptr() + 2))) == -1
        torch.cuda.synchronize()
