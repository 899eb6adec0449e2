"""alacgpu_kaldi_pitch_device on two streams: all three launches of a call go through the context's shared scratch -- the
downsampled rows, the NCCF planes and the backpointers --, which its calls use one after the other whatever their streams.  Two
calls with different inputs on two streams of one context are each their own single-stream result, back to back, with no host
wait between them.  The calls are made as tests/stage_stream_calls.py makes the other stages'."""
import numpy as np
import pytest

from stage_stream_calls import CFG, Call, alone, same_bits

pytestmark = pytest.mark.gpu

ROUNDS = 8


def pitch_call(torch, pkg, seed, rows=3, channels=2, frames=3000):
    from alac.net_amd.kaldi_pitch import _table_device
    from test_yin_spec import voiced_noise

    spec = pkg.KaldiPitch(16000, min_f0=100, max_f0=300, delta_pitch=0.01)
    rng = np.random.default_rng(500 + seed)
    true = dict(x=torch.from_numpy(voiced_noise(rows, channels, frames, 16000, seed=500 + seed)).to("cuda"),
                valid=torch.from_numpy(rng.integers(frames // 2, frames + 1, rows)).to("cuda"))
    n = int(spec.frames(frames))
    outs = [torch.empty((rows, channels, spec.lines, n), dtype=torch.float32, device="cuda")]
    table = _table_device(spec, torch.device("cuda", torch.cuda.current_device()))
    t = spec.tables()
    torch.cuda.synchronize()

    def fn(ctx, b, o, stream):
        ctx.kaldi_pitch_device(b["x"], rows, channels, frames, frames, b["valid"], spec.sample_rate, spec.resample_freq, spec.win_length,
                               spec.hop_length, spec.window, spec.shift, spec.first_lag, spec.last_lag, spec.n_states, spec.phases,
                               spec.in_per_unit, t["down"].shape[1], t["up"].shape[1], spec.flags, spec.normalization_left_context,
                               spec.normalization_right_context, spec.delta_window, table, None, None, o[0], n, stage=0, stream=stream)

    return Call(torch, true, outs, fn, wrong=dict(valid=frames))


def test_two_calls_on_two_streams_share_the_scratch_and_are_each_their_own():
    import torch

    import alac.net_amd as pkg

    A, B = pitch_call(torch, pkg, 1), pitch_call(torch, pkg, 2)
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
