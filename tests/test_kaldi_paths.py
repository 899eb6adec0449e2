"""alacgpu_fbank_device and alacgpu_mfcc_device by code path, as tests/test_features_paths.py does it for the log-mel kernel: the
grid PATHS of tests/test_fbank_spec.py (one shape per branch of alac_fbank.hip and alac_mfcc.hip that depends on the tile, the
lane or the skew) against the specification and its float32 twin, many tiles of many planes with every frame compared,
properties that need no tolerance (a frame does not depend on where it sits, nor a plane on its neighbours), and the
reflection where it crosses tiles.  The checks and the harness are those of tests/test_fbank.py and tests/test_mfcc.py: NaNs
behind every plane, the output prefilled with NaN between guards.  tests/test_fbank_spec.py and tests/test_mfcc_spec.py hold
on the CPU what the checks rest on (the twin inside the bound, the narrow share, dC <= 1) for the same shapes."""
import numpy as np
import pytest

from test_fbank import check_log, check_power, gpu, noise  # noqa: F401
from test_fbank import run_kernel as run_fbank
from test_fbank import spec_of as fbank_spec
from test_fbank_spec import PATHS, paths_length
from test_features import kernel_tile
from test_mfcc import check_bound, check_dct_of_fbank, fbank_of  # noqa: F401
from test_mfcc import run_kernel as run_mfcc
from test_mfcc import spec_of as mfcc_spec

pytestmark = pytest.mark.gpu

KINDS = ("fbank", "mfcc")
TWO_CHANNELS = [(63, 7), (401, 161)]
TILES = {(2048, 600): 30, (2048, 2048): 9}         # the shapes of PATHS whose tile is not 32
WIDEST = (2048, 560, 256, 23)                      # dC reaches 3.4 there (tests/test_mfcc_spec.py): the bound would be vacuous
ENERGY = (dict(use_energy=True, raw_energy=True), dict(use_energy=True, raw_energy=False))


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def centred_length(hop, frames):
    """A short L with `frames` frames without snip_edges"""
    return frames * hop - hop // 2 + min(3, hop - 1)


def test_the_tiles_of_the_grid():
    for win, hop, _, _, frames in PATHS:
        tile = kernel_tile(win, hop)
        assert tile == TILES.get((win, hop), 32), (win, hop, tile)
        assert frames > tile                                          # every case has a second tile


@pytest.mark.parametrize("snip", [True, False])
@pytest.mark.parametrize("win,hop,n_mels,n_ceps,frames", PATHS)
@pytest.mark.parametrize("kind", KINDS)
def test_grid_equals_the_specification(gpu, kind, win, hop, n_mels, n_ceps, frames, snip):
    """Two rows (one at 2048 taps), two channels on the two odd shapes.  At 2048 taps the twin's ratio is left to the CPU files
    (both references of 63 frames take 15 s there); the bound, every element, stays."""
    torch, pkg, ctx = gpu
    L = paths_length(win, hop, frames)
    x = noise(np.random.default_rng(win + hop), 1 if win == 2048 else 2, 2 if (win, hop) in TWO_CHANNELS else 1, L)
    tag = f"{kind} ({win},{hop},{n_mels},{n_ceps}) L {L} x{x.shape[1]} snip {snip}"
    twin = win != 2048
    if kind == "fbank":
        power = fbank_spec(win, hop, n_mels, snip_edges=snip, log=False)
        assert power.frames(L) == frames or not snip
        got, intact = run_fbank(torch, ctx, x, power)
        assert intact, tag
        M, dM = check_power(got, x, power, tag, twin=twin)
        got, intact = run_fbank(torch, ctx, x, fbank_spec(win, hop, n_mels, snip_edges=snip))
        assert intact, tag
        check_log(got, M, dM, tag)
        return
    spec = mfcc_spec(win, hop, n_mels, n_ceps, snip_edges=snip)
    got, intact = run_mfcc(torch, ctx, x, spec)
    assert intact, tag
    if (win, hop, n_mels, n_ceps) == WIDEST:
        # no dC here: what holds the cepstra is the DCT of the fbank kernel's bits below, which the fbank case of this shape
        # holds to its own bound
        assert got.shape == (1, 1, n_ceps, spec.frames(L)) and np.isfinite(got).all(), tag
    else:
        check_bound(got, x, spec, tag, twin=twin)
    F, intact = run_mfcc(torch, ctx, x, spec, fbank=True)
    assert intact, tag
    check_dct_of_fbank(got, F, spec, tag)


@pytest.mark.parametrize("snip", [True, False])
@pytest.mark.parametrize("win,hop,n_mels,n_ceps", [(400, 160, 80, 13), (63, 7, 12, 12)])
@pytest.mark.parametrize("kind", KINDS)
def test_many_tiles_every_frame(gpu, kind, win, hop, n_mels, n_ceps, snip):
    """Five tiles (four full ones and seven frames) of three rows of two channels: 30 workgroups, plane and tile index both
    above zero at once, and five is odd, so every rotation of the waves (blockIdx.x & 3) meets every tile index; every frame
    of every tile is held against the specification and the twin.  MFCC with the energy of the windowed frame, which reads a
    predecessor in its own pass."""
    torch, pkg, ctx = gpu
    tile = kernel_tile(win, hop)
    T = 4 * tile + 7
    L = paths_length(win, hop, T) if snip else centred_length(hop, T)
    assert len({(b & 3, b % 5) for b in range(3 * 2 * 5)}) == 4 * 5           # blockIdx.x = plane * tiles + tile index
    x = noise(np.random.default_rng(hop), 3, 2, L)
    tag = f"{kind} ({win},{hop},{n_mels}) 5 tiles x 3 x 2 snip {snip}"
    if kind == "fbank":
        power = fbank_spec(win, hop, n_mels, snip_edges=snip, log=False)
        assert power.frames(L) == T
        got, intact = run_fbank(torch, ctx, x, power)
        assert intact, tag
        M, dM = check_power(got, x, power, tag, twin=True)
        got, intact = run_fbank(torch, ctx, x, fbank_spec(win, hop, n_mels, snip_edges=snip))
        assert intact, tag
        check_log(got, M, dM, tag)
    else:
        spec = mfcc_spec(win, hop, n_mels, n_ceps, snip_edges=snip, use_energy=True, raw_energy=False)
        assert spec.frames(L) == T
        got, intact = run_mfcc(torch, ctx, x, spec)
        assert intact, tag
        check_bound(got, x, spec, tag, twin=True)
        F, intact = run_mfcc(torch, ctx, x, spec, fbank=True)
        assert intact, tag
        check_dct_of_fbank(got, F, spec, tag)


def transforms(win, hop, n_mels, n_ceps, snip):
    """(tag, run, spec): fbank with and without the log, MFCC with either energy"""
    for log in (False, True):
        yield f"fbank log {log}", run_fbank, fbank_spec(win, hop, n_mels, snip_edges=snip, log=log)
    for kw in ENERGY:
        yield f"mfcc {kw}", run_mfcc, mfcc_spec(win, hop, n_mels, n_ceps, snip_edges=snip, **kw)


@pytest.mark.parametrize("snip", [True, False])
@pytest.mark.parametrize("win,hop,n_mels,n_ceps", [(400, 160, 23, 13), (64, 16, 8, 8), (63, 7, 12, 12), (16, 1, 4, 4), (2048, 600, 40, 20)])
def test_a_frame_does_not_depend_on_where_it_sits(gpu, win, hop, n_mels, n_ceps, snip):
    """f(x[k hop:])[..., t] == f(x)[..., t + k] bit for bit, k a tile and five frames: another lane, another tile, another
    wave rotation, another slot of the means and the energies do the same arithmetic.  With snip_edges nothing reflects and
    every frame is compared; without, every frame whose window is inside both signals.  The energy line is one of the lines."""
    torch, pkg, ctx = gpu
    tile = kernel_tile(win, hop)
    k = tile + 5
    tail = win + (tile + 9) * hop
    x = noise(np.random.default_rng(win + hop), 2, 1, k * hop + tail)
    for tag, run, spec in transforms(win, hop, n_mels, n_ceps, snip):
        t = np.arange(spec.frames(tail))
        first = 0 if snip else hop // 2 - win // 2
        ok = (t * hop + first >= 0) & (t * hop + first + win <= tail)
        assert ok.all() if snip else (ok.sum() >= 8 and not ok[0]), tag
        assert len(t) > tile and k % tile == 5
        whole, intact = run(torch, ctx, x, spec)
        assert intact, tag
        part, intact = run(torch, ctx, np.ascontiguousarray(x[:, :, k * hop:]), spec)
        assert intact and part.shape[-1] == len(t) and whole.shape[-1] == len(t) + k, tag
        assert np.isfinite(part).all() and np.isfinite(whole).all(), tag
        assert np.array_equal(bits(part[..., ok]), bits(whole[..., t[ok] + k])), (win, hop, tag)
        if not snip:                                                  # (the first frame reflects: the test can fail)
            assert not np.array_equal(bits(part[..., 0]), bits(whole[..., k])), tag


@pytest.mark.parametrize("snip", [True, False])
@pytest.mark.parametrize("kind,win,hop,n_mels,n_ceps,frames", [("fbank",) + PATHS[6], ("mfcc",) + PATHS[1], ("mfcc",) + PATHS[3]])
def test_a_batch_is_its_planes_run_alone(gpu, kind, win, hop, n_mels, n_ceps, frames, snip):
    torch, pkg, ctx = gpu
    assert PATHS[6][:3] == (2048, 560, 256) and PATHS[1][:2] == (401, 161) and PATHS[3][:2] == (16, 16)
    x = noise(np.random.default_rng(frames), 3, 2, paths_length(win, hop, frames))
    if kind == "fbank":
        cases = [(run_fbank, fbank_spec(win, hop, n_mels, snip_edges=snip, log=log)) for log in (False, True)]
    else:
        cases = [(run_mfcc, mfcc_spec(win, hop, n_mels, n_ceps, snip_edges=snip, **kw)) for kw in ENERGY]
    for run, spec in cases:
        whole, intact = run(torch, ctx, x, spec)
        assert intact and np.isfinite(whole).all() and whole.shape[-1] > kernel_tile(win, hop)
        for r in range(3):
            for c in range(2):
                one, intact = run(torch, ctx, x[r:r + 1, c:c + 1], spec)
                assert intact and np.array_equal(bits(one[0, 0]), bits(whole[r, c])), (kind, r, c)


@pytest.mark.parametrize("win,hop,n_mels,n_ceps", [(400, 160, 80, 13), (63, 7, 12, 12)])
@pytest.mark.parametrize("kind", KINDS)
def test_reflection_across_tiles(gpu, kind, win, hop, n_mels, n_ceps):
    """Without snip_edges.  The shortest L of two tiles and one frame: the last frame is alone in the third tile and reflects
    behind L.  Then two rows of fewer than half a window's samples, where every tap of every frame is reflected, on both
    sides.  Both against the bound.  A NaN at sample L - 1 reaches exactly the frames `fbank_frame_index` names -- in the
    long row they lie in two tiles -- and every other frame, of every tile, is bit for bit the clean run's."""
    torch, pkg, ctx = gpu
    from alac.net_amd.fbank import fbank_frame_index

    tile = kernel_tile(win, hop)
    if kind == "fbank":
        run, spec = run_fbank, fbank_spec(win, hop, n_mels, snip_edges=False, log=False)
        check = lambda got, x, tag: check_power(got, x, spec, tag)
    else:
        run, spec = run_mfcc, mfcc_spec(win, hop, n_mels, n_ceps, snip_edges=False, use_energy=True)
        check = lambda got, x, tag: check_bound(got, x, spec, tag)
    rng = np.random.default_rng(win)
    long = (2 * tile + 1) * hop - hop // 2
    short = win // 2 - 1
    for rows, L in ((1, long), (2, short)):
        x = noise(rng, rows, 1, L) + np.float32(0.25)
        idx = fbank_frame_index(L, spec)
        T = idx.shape[0]
        g = np.arange(T)[:, None] * hop + hop // 2 - win // 2 + np.arange(win)[None, :]       # before the reflection
        if L == long:
            assert T == 2 * tile + 1 and g[-1].max() >= L and spec.frames(L - 1) == T - 1
        else:
            assert T >= 1 and (g.min(axis=1) < 0).all() and (g.max(axis=1) >= L).all()
        tag = f"{kind} ({win},{hop}) L {L} reflected"
        clean, intact = run(torch, ctx, x, spec)
        assert intact and clean.shape[-1] == T, tag
        check(clean, x, tag)
        y = x.copy()
        y[-1, 0, L - 1] = np.nan
        hit = (idx == L - 1).any(axis=1)
        assert hit.any() and (L == short or (not hit.all() and len(set(np.flatnonzero(hit) // tile)) == 2)), tag
        dirty, intact = run(torch, ctx, y, spec)
        assert intact, tag
        assert np.isnan(dirty[-1, 0][:, hit]).all(), tag
        assert np.array_equal(bits(dirty[-1, 0][:, ~hit]), bits(clean[-1, 0][:, ~hit])), tag
        assert np.array_equal(bits(dirty[:-1]), bits(clean[:-1])), tag
