"""alacgpu_pcen_device on two streams: the call uses nothing of the context but its device -- no scratch, no atomics -- so two
calls with different inputs on two streams of one context are each their own single-stream result, back to back, with no host
wait between them.  The calls are made as tests/test_yin_streams.py makes its own: a `Call` whose inputs are loaded on the
stream that runs it and whose outputs are cloned on it behind the call, and whose reference is the same call alone on a fresh
context."""
import numpy as np
import pytest

from stage_stream_calls import CFG, Call, alone, same_bits

pytestmark = pytest.mark.gpu

ROUNDS = 16


def pcen_call(torch, pkg, seed, rows=3, lines=6, frames=1500):
    """A per-bin pcen call over rows of different lengths on lines of two passes of the workgroup team: the energies, the
    lengths and the table are inputs the call reads on its stream"""
    from test_pcen_spec import energies

    rng = np.random.default_rng(500 + seed)
    how = pkg.Pcen(rng.uniform(0.01, 0.2, 3).tolist(), gain=rng.uniform(0.5, 1.0, 3).tolist(), power=[0.5, 0.4, 0.3])
    true = dict(x=torch.from_numpy(energies((rows, lines, frames), 500 + seed)).to("cuda"),
                valid=torch.from_numpy(rng.integers(frames // 2, frames + 1, rows)).to("cuda"),
                table=torch.from_numpy(how.table()).to("cuda"))
    outs = [torch.empty((rows, lines, frames), dtype=torch.float32, device="cuda")]

    def fn(ctx, b, o, stream):
        ctx.pcen_device(b["x"], o[0], rows, lines, frames, frames, b["valid"], 0.0, 0.0, 0.0, 0.0, 0.0, how.eps, how.scale, d_table=b["table"],
                        lines_per_param=3, stream=stream)

    return Call(torch, true, outs, fn, wrong=dict(valid=frames))


def test_two_calls_on_two_streams_are_each_their_own():
    import torch

    import alac.net_amd as pkg

    A, B = pcen_call(torch, pkg, 1), pcen_call(torch, pkg, 2)
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
