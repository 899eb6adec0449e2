"""alacgpu_pyin_device on two streams: both launches of a call go through the context's shared scratch -- the observations and
the backpointers --, which its calls use one after the other whatever their streams.  Two calls with different inputs on two
streams of one context are each their own single-stream result, back to back, with no host wait between them.  The calls are
made as tests/stage_stream_calls.py makes the other stages'."""
import numpy as np
import pytest

from stage_stream_calls import CFG, Call, alone, same_bits

pytestmark = pytest.mark.gpu

ROUNDS = 16


def pyin_call(torch, pkg, seed, rows=3, channels=2, frames=3000):
    from alac.net_amd.pyin import _table_device
    from test_yin_spec import voiced_noise

    spec = pkg.PYin(16000, 128, 80, 100.0, 400.0, resolution=0.5)
    rng = np.random.default_rng(400 + seed)
    true = dict(x=torch.from_numpy(voiced_noise(rows, channels, frames, 16000, seed=400 + seed)).to("cuda"),
                valid=torch.from_numpy(rng.integers(frames // 2, frames + 1, rows)).to("cuda"))
    n = int(spec.frames(frames))
    outs = [torch.empty((rows, channels, 3, n), dtype=torch.float32, device="cuda")]
    table = _table_device(spec, torch.device("cuda", torch.cuda.current_device()))
    torch.cuda.synchronize()

    def fn(ctx, b, o, stream):
        ctx.pyin_device(b["x"], rows, channels, frames, frames, b["valid"], spec.sample_rate, spec.win_length, spec.hop_length,
                        spec.tau_min, spec.tau_max, 0, spec.n_thresholds, spec.n_bins, spec.band, spec.no_trough_prob, table, None,
                        None, None, o[0], None, n, stage=0, stream=stream)

    return Call(torch, true, outs, fn, wrong=dict(valid=frames))


def test_two_calls_on_two_streams_share_the_scratch_and_are_each_their_own():
    import torch

    import alac.net_amd as pkg

    A, B = pyin_call(torch, pkg, 1), pyin_call(torch, pkg, 2)
    wantA, wantB = alone(torch, pkg, A), alone(torch, pkg, B)
    assert not same_bits(torch, wantA, wantB)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    with pkg.AlacGpuContext(CFG) as ctx:
        gotA, gotB = [], []
        for _ in range(ROUNDS):
            for call, s, got in ((A, s1, gotA), (B, s2, gotB)):
                with torch.cuda.stream(s):
                    call.poison()
                    call.load()
                    call.run(ctx, s.cuda_stream)
                    got.append(call.clones())
        torch.cuda.synchronize()
    for r in range(ROUNDS):
        assert same_bits(torch, gotA[r], wantA) and same_bits(torch, gotB[r], wantB), r
