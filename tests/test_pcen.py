"""alacgpu_pcen_device on the GPU: stage 1 bit for bit the smoother's float32 twin (pcen.pcen_smoother_host_f32), stage 0 bit for
bit the full twin (pcen.pcen_host_f32), zeros comparing equal, and within the derived bound dY of the specification
(pcen.pcen_host); then `pcen` and `normalize` with a Pcen.

The harness is tests/test_sliding.py's: every call reads source lines that carry NaN behind line_len and writes into an output
prefilled with NaN between guards of 0x5A bytes; the guards, what lies behind line_len and, when not in place, the source are
checked after every call.  Shapes are chosen by code path from csrc/alac_pcen.h: lines of one and two frames, both sides of a
lane's chunk, of a pass of the wave team and of two, both sides of the threshold between the teams -- which is where the
workgroup team's pass ends --, two of its passes and a frame, and one shape of twenty passes and three frames."""
import importlib

import numpy as np
import pytest

from test_features import header_constant
from test_normalize_spec import same_bits
from test_pcen_spec import energies

pytestmark = pytest.mark.gpu

GUARD = 64
SLACK = 5
ROWS = 9                 # the eight lengths of `valid_for` and the first again
LINES = 3                # 27 lines: not a multiple of the wave team's lines per workgroup


def constant(name):
    return header_constant(name, "alac_pcen.h")


@pytest.fixture(scope="module")
def gpu():
    import torch

    import alac.net_amd as pkg

    assert (ROWS * LINES) % constant("ALAC_PCEN_WAVE_LINES")
    with pkg.AlacGpuContext([(4096, 16, 40, 10, 14, 2)], device=0) as ctx:
        yield torch, ctx


def run(gpu, x, how, valid=None, stage=0, slack=SLACK, in_place=False):
    """One alacgpu_pcen_device call over x [rows, lines_per_row, n], as tests/test_sliding.py's run; a per-bin `how` goes as
    its table"""
    torch, ctx = gpu
    dev = torch.device("cuda", 0)
    rows, lpr, n = x.shape
    S = n + slack
    src = np.full((rows, lpr, S), np.nan, dtype=np.float32)
    src[:, :, :n] = x
    total = rows * lpr * S
    raw = torch.full(((total + 2 * GUARD) * 4,), 0x5A, dtype=torch.uint8, device=dev).view(torch.float32)
    out = raw[GUARD:GUARD + total]
    d_src = torch.from_numpy(src).to(dev)
    if in_place:
        out.copy_(d_src.flatten())
        d_src = out
    else:
        out.fill_(float("nan"))
    d_valid = None if valid is None else torch.tensor(list(valid), dtype=torch.int64, device=dev)
    table = how.table()
    stream = torch.cuda.current_stream().cuda_stream
    if how.lines is None:
        ctx.pcen_device(d_src, out, rows, lpr, S, n, d_valid, *(float(a) for a in table[:, 0]), how.eps, how.scale, stage=stage, stream=stream)
    else:
        ctx.pcen_device(d_src, out, rows, lpr, S, n, d_valid, 0.0, 0.0, 0.0, 0.0, 0.0, how.eps, how.scale,
                        d_table=torch.from_numpy(table).to(dev), lines_per_param=how.lines, stage=stage, stream=stream)
    torch.cuda.synchronize()
    assert bool((torch.cat([raw[:GUARD], raw[GUARD + total:]]).view(torch.uint8) == 0x5A).all()), "a guard was written"
    got = out.cpu().numpy().reshape(rows, lpr, S)
    if slack:
        assert np.isnan(got[:, :, n:]).all(), "an element behind line_len was written"
    if not in_place:
        back = d_src.cpu().numpy()
        assert np.array_equal(back[:, :, :n], x, equal_nan=True) and np.isnan(back[:, :, n:]).all(), "the source was written"
    return got[:, :, :n].copy()


def as_bins(x, how):
    """x [rows, lines, n] as the [rows, C, L, n] a per-bin specification is stated on"""
    return x if how.lines is None else x.reshape(x.shape[0], -1, how.lines, x.shape[-1])


def check(gpu, x, how, valid, tag, **kw):
    """Both stages of one input against the twins, and stage 0 against the specification"""
    from alac.net_amd.pcen import pcen_host, pcen_host_f32, pcen_smoother_host_f32

    xb = as_bins(x, how)
    got = run(gpu, x, how, valid, stage=1, **kw)
    want = pcen_smoother_host_f32(xb, how, valid).reshape(x.shape)
    assert same_bits(got, want), (tag, "the smoother is not its twin", int(np.argmax(~((got == want) | (np.isnan(got) & np.isnan(want))))))
    got = run(gpu, x, how, valid, stage=0, **kw)
    want = pcen_host_f32(xb, how, valid).reshape(x.shape)
    assert same_bits(got, want), (tag, "not the twin", int(np.argmax(~((got == want) | (np.isnan(got) & np.isnan(want))))))
    y, dY = (a.reshape(x.shape) for a in pcen_host(xb, how, valid, bound=True))
    ok = np.isfinite(y)
    assert np.array_equal(np.isfinite(got), ok), (tag, "not finite where the specification is, or the reverse")
    err = np.abs(got.astype(np.float64)[ok] - y[ok])
    assert (err <= dY[ok]).all(), (tag, float((err / np.maximum(dY[ok], 1e-300)).max()))
    return got


def valid_for(n, turn=0):
    pool = [n + 5, 1, -1, n, 0, n // 2, n - 1, 2]
    return [pool[(turn + r) % len(pool)] for r in range(ROWS)]


def lengths_by_path():
    chunk, wave_max, line = constant("ALAC_PCEN_CHUNK"), constant("ALAC_PCEN_WAVE_MAX"), constant("ALAC_PCEN_LINE_THREADS")
    wave_pass, line_pass = 64 * chunk, line * chunk
    assert wave_max % wave_pass == 0 and wave_max >= 2 * wave_pass + 1 and line_pass >= wave_max
    return sorted({1, 2, chunk - 1, chunk, chunk + 1, wave_pass - 1, wave_pass, wave_pass + 1, 2 * wave_pass + 1, wave_max - 1, wave_max,
                   wave_max + 1, line_pass - 1, line_pass, line_pass + 1, 2 * line_pass + 1})


@pytest.mark.parametrize("n", lengths_by_path())
def test_pcen_grid(gpu, n):
    from alac.net_amd.pcen import Pcen

    for turn, how in enumerate((Pcen(frame_rate=100.0), Pcen(0.3, gain=0.5, bias=10.0, power=0.25, eps=1e-3, scale=2.0 ** 31))):
        x = energies((ROWS, LINES, n), 100 * n + turn, scale=(1.0, 2.0 ** -31)[turn])
        check(gpu, x, how, valid_for(n, turn), f"n {n} {how}", in_place=bool(turn))
    x = energies((2, LINES, n), n + 7, scale=1e-6)
    check(gpu, x, Pcen(frame_rate=62.5), None, f"n {n} whole lines", slack=0)


def test_a_line_of_twenty_passes_and_three_frames(gpu):
    from alac.net_amd.pcen import Pcen

    n = 20 * constant("ALAC_PCEN_LINE_THREADS") * constant("ALAC_PCEN_CHUNK") + 3
    x = energies((ROWS, 1, n), 20)
    how = Pcen(frame_rate=100.0)
    ref = check(gpu, x, how, valid_for(n), f"n {n}")
    assert same_bits(run(gpu, x, how, valid_for(n), in_place=True), ref)


def test_in_place_rows_alone_and_strides_change_nothing(gpu):
    from alac.net_amd.pcen import Pcen

    wave = constant("ALAC_PCEN_WAVE_MAX")
    how = Pcen(frame_rate=100.0)
    for k, n in enumerate((201, wave - 55, wave + 300, 3001)):
        x = energies((3, 5, n), 70 + k)
        valid = [n - 7, -1, n // 2]
        for stage in (1, 0):
            ref = run(gpu, x, how, valid, stage=stage)
            assert same_bits(run(gpu, x, how, valid, stage=stage, in_place=True), ref), (n, stage, "in place")
            assert same_bits(run(gpu, x, how, valid, stage=stage, slack=0), ref), (n, stage, "line_stride == line_len")
            assert same_bits(run(gpu, x, how, valid, stage=stage, slack=0, in_place=True), ref), (n, stage, "in place, line_stride == line_len")
        for r in range(3):
            assert same_bits(run(gpu, x[r:r + 1], how, valid[r:r + 1])[0], ref[r]), (n, "row alone", r)


@pytest.mark.parametrize("bins", [1, 3])
def test_per_bin_tables_under_two_channels(gpu, bins):
    from alac.net_amd.pcen import Pcen

    rng = np.random.default_rng(bins)
    how = Pcen(rng.uniform(0.01, 0.5, bins).tolist(), gain=rng.uniform(0.3, 1.0, bins).tolist(), bias=rng.uniform(0.0, 5.0, bins).tolist(),
               power=rng.uniform(0.1, 1.0, bins).tolist(), eps=1e-5)
    wave = constant("ALAC_PCEN_WAVE_MAX")
    for n in (201, wave + 77):
        x = energies((3, 2 * bins, n), n + bins)
        valid = [n, n // 2, -1]
        got = check(gpu, x, how, valid, f"bins {bins} n {n}")
        # every bin is the scalar call on its own lines
        for j in range(bins):
            one = Pcen(how.b[j], gain=how.gain[j], bias=how.bias[j], power=how.power[j], eps=1e-5)
            lines = [j, bins + j]
            assert same_bits(run(gpu, np.ascontiguousarray(x[:, lines[:1]]), one, valid), got[:, lines[:1]]), (bins, n, j)
            assert same_bits(run(gpu, np.ascontiguousarray(x[:, lines[1:]]), one, valid), got[:, lines[1:]]), (bins, n, j)


def test_what_is_not_finite_goes_forward_in_its_own_line_only(gpu):
    from alac.net_amd.pcen import Pcen

    wave = constant("ALAC_PCEN_WAVE_MAX")
    how = Pcen(frame_rate=100.0)
    for n in (wave - 56, wave + 200):
        v, at = n - 7, n // 3
        valid = [v, -1, n, v]
        for bad in (np.nan, np.inf):
            x = energies((4, 2, n), 9)
            x[0, 1, at] = bad              # at t
            x[0, 0, v] = np.nan            # at v
            x[0, 0, n - 1] = np.inf        # behind v; behind line_len the harness has NaN throughout
            x[1] = np.nan                  # a length of -1: nothing of the row is read
            x[3, 0, v - 1] = bad           # at v - 1
            for in_place in (False, True):
                M = run(gpu, x, how, valid, stage=1, in_place=in_place)
                got = check(gpu, x, how, valid, f"n {n} {bad}", in_place=in_place)
                reached = np.zeros(n, dtype=bool)
                reached[at:v] = True
                assert np.array_equal(~np.isfinite(M[0, 1]), reached), (n, bad)
                if bad is np.nan:
                    assert np.array_equal(np.isnan(got[0, 1]), reached), (n, bad)
                else:                       # s / inf^gain is 0 again behind the infinity
                    assert np.isnan(got[0, 1, at]) and np.isfinite(got[0, 1, :at]).all() and np.isfinite(got[0, 1, at + 1:]).all()
                for res in (M, got):
                    assert np.isfinite(res[0, 0]).all() and (res[1] == 0).all() and np.isfinite(res[2]).all()
                    assert not np.isfinite(res[3, 0, v - 1]) and np.isfinite(res[3, 0, :v - 1]).all() and (res[3, :, v:] == 0).all()
                    assert np.isfinite(res[3, 1]).all()
    # a negative energy, and zeros throughout
    x = energies((1, 2, 300), 10)
    x[0, 0, 100] = -40.0
    got = check(gpu, x, how, None, "a negative energy")
    assert np.isnan(got[0, 0, 100]) and np.isfinite(got[0, 1]).all()
    got = check(gpu, np.zeros((2, 3, 300), dtype=np.float32), how, [300, 150], "zeros")
    assert (np.abs(got) <= 2.0 ** -22 * 2.0 ** 0.5).all()


def test_bad_arguments_are_refused_before_anything_is_enqueued(gpu):
    import ctypes as C

    import alac.net_amd as pkg

    torch, ctx = gpu
    rows, lpr, S, n = 2, 6, 40, 36
    src = torch.zeros(rows * lpr * S, device="cuda")
    out = torch.full((rows * lpr * S,), 7.0, device="cuda")
    valid = torch.zeros(rows, dtype=torch.int64, device="cuda")
    table = torch.full((5, 3), 0.5, device="cuda")
    p = lambda t, off=0: C.c_void_p(t.data_ptr() + off)
    nan, inf = float("nan"), float("inf")
    good = dict(src=p(src), out=p(out), rows=rows, lpr=lpr, S=S, n=n, valid=p(valid), b=0.1, gain=0.98, bias=2.0, power=0.5, c=2.0 ** 0.5,
                eps=1e-6, scale=1.0, table=None, lpp=0, stage=0)
    bad = [dict(src=None), dict(out=None), dict(src=p(src, 2)), dict(out=p(out, 1)), dict(valid=p(valid, 4)), dict(lpr=0), dict(n=0),
           dict(n=S + 1), dict(out=p(src, 4)), dict(out=p(src, 4 * ((rows * lpr - 1) * S + n - 1))), dict(rows=1 << 31, S=1 << 20, n=300),
           dict(b=0.0), dict(b=1.5), dict(b=nan), dict(gain=-1.0), dict(gain=inf), dict(bias=-1.0), dict(bias=nan), dict(power=0.0),
           dict(power=inf), dict(c=-1.0), dict(c=nan), dict(eps=0.0), dict(eps=inf), dict(scale=0.0), dict(scale=nan), dict(stage=2),
           dict(stage=-1), dict(table=p(table), lpp=0), dict(table=p(table), lpp=4), dict(table=p(table, 2), lpp=3)]
    call = lambda a: pkg.lib().alacgpu_pcen_device(ctx._ctx, a["src"], a["out"], a["rows"], a["lpr"], a["S"], a["n"], a["valid"], a["b"],
                                                   a["gain"], a["bias"], a["power"], a["c"], a["eps"], a["scale"], a["table"], a["lpp"],
                                                   a["stage"], None)
    for change in bad:
        assert call({**good, **change}) == -1, change
    torch.cuda.synchronize()
    assert (out == 7.0).all()
    assert call({**good, "rows": 0}) == 0 and call({**good, "valid": None, "out": p(src)}) == 0
    assert call({**good, "out": p(src), "table": p(table), "lpp": 3, "b": nan}) == 0            # (the scalars are not looked at)
    torch.cuda.synchronize()
    assert (out == 7.0).all()


def test_the_public_calls(gpu):
    import alac.net_amd as pkg

    torch, _ = gpu
    x = energies((3, 2, 5, 298), 4)
    d = torch.from_numpy(x).cuda()
    lengths = [298, 123, -1]
    per_bin = pkg.Pcen([0.02, 0.03, 0.05, 0.1, 0.2], gain=[0.98, 0.9, 0.8, 0.7, 0.6], bias=2.0, power=[0.5, 0.5, 0.4, 0.3, 0.2])
    for how in (pkg.Pcen(frame_rate=100.0), per_bin):
        want = pkg.normalize_host_f32(x, how, lengths)
        assert same_bits(want, pkg.pcen_host_f32(x, how, lengths))
        got = pkg.pcen(d, how, lengths)
        assert got.shape == d.shape and got.data_ptr() != d.data_ptr() and torch.equal(d.cpu(), torch.from_numpy(x))
        assert same_bits(got.cpu().numpy(), want), how
        assert torch.equal(pkg.normalize(d, how, lengths), got)
        assert torch.equal(pkg.pcen(d, how, torch.tensor(lengths, device="cuda")), got)
        e = d.clone()
        assert pkg.normalize(e, how, lengths, out=e) is e and torch.equal(e, got)
        e = d.clone()
        assert pkg.pcen(e, how, lengths, out=e) is e and torch.equal(e, got)
    tables = importlib.import_module("alac.net_amd.pcen")._TABLES           # the table is uploaded once per (spec, device) and kept
    kept = [t for (spec, _), t in tables.items() if spec == per_bin]
    assert len(kept) == 1 and kept[0].is_cuda and kept[0].shape == (5, 5)
    pkg.pcen(d, pkg.Pcen(per_bin.b, gain=per_bin.gain, bias=2.0, power=per_bin.power), lengths)      # an equal spec: the same table
    assert [t for (spec, _), t in tables.items() if spec == per_bin][0] is kept[0] and len(tables) <= 64
    how = pkg.Pcen(frame_rate=100.0)
    assert same_bits(pkg.pcen(d[:, 0].contiguous(), how, lengths).cpu().numpy(), pkg.pcen_host_f32(x, how, lengths)[:, 0])     # [B, lines, n]
    # the slice [..., :297]: the last column is neither read nor written
    z = x.copy()
    z[..., 297] = np.nan
    for how in (how, per_bin):
        dz = torch.from_numpy(z).cuda()
        want = pkg.pcen_host_f32(np.ascontiguousarray(x[..., :297]), how, [297, 123, -1])
        assert pkg.normalize(dz[..., :-1], how, [297, 123, -1], out=dz[..., :-1]).data_ptr() == dz.data_ptr()
        back = dz.cpu().numpy()
        assert same_bits(back[..., :297], want) and np.isnan(back[..., 297]).all()
    assert pkg.pcen(d[:0], how).shape == (0, 2, 5, 298)
    for args in ((d.cpu(), how), (d.double(), how), (d[..., ::2], how), (d, how, [1, 2]), (d, pkg.MeanVar()), (d[:, :, :4], per_bin),
                 (d[:, 0], per_bin)):
        with pytest.raises(ValueError):
            pkg.pcen(*args)
    with pytest.raises(ValueError):
        pkg.normalize(d[:, 0], per_bin)
