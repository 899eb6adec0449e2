"""alacgpu_rir_shoebox_device on two streams: the call uses nothing of the context but its device -- no scratch, no atomics --
so two calls with different rooms on two streams of one context are each their own single-stream result, back to back, with
no host wait between them.  Built on tests/stage_stream_calls.py as tests/test_cqt_streams.py is: a `Call` whose input is
loaded on the stream that runs it and whose output is cloned on it behind the call, and whose reference is the same call
alone on a fresh context."""
import numpy as np
import pytest

from stage_stream_calls import CFG, Call, alone, same_bits

pytestmark = pytest.mark.gpu

ROUNDS = 8
K = 300


def rir_call(torch, seed):
    rng = np.random.default_rng(seed)
    L = rng.uniform([3, 3, 2.5], [6, 5, 3.5], size=(3, 3))
    g = np.concatenate([L, L * rng.uniform(0.1, 0.9, size=(3, 3)), L * rng.uniform(0.1, 0.9, size=(3, 3))], axis=1)
    true = dict(geometry=torch.from_numpy(g).cuda(), beta=torch.from_numpy(rng.uniform(0.5, 0.95, size=(3, 6)).astype(np.float32)).cuda())
    outs = [torch.empty((3, 1, K), dtype=torch.float32, device="cuda"), torch.empty(3, dtype=torch.int32, device="cuda")]

    def fn(ctx, b, o, stream):
        ctx.rir_shoebox_device(b["geometry"], b["beta"], 3, 8000, K, 81, -1, 343.0, o[0], K, o[1], stream=stream)

    return Call(torch, true, outs, fn)


def test_two_calls_on_two_streams_are_each_their_own():
    import torch

    import alac.net_amd as pkg

    A, B = rir_call(torch, 1), rir_call(torch, 2)
    wantA, wantB = alone(torch, pkg, A), alone(torch, pkg, B)
    assert not same_bits(torch, wantA, wantB) and wantA[1].tolist() == [K] * 3
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
