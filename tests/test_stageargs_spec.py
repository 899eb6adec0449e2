"""The one argument check of the stage calls that change a signal by a companion per row (alac.net_amd/_stageargs.py):
every refusal of `mix` and `reverb` in front of their library call, by its message, and what the check hands on.  CPU only:
the tensors are host tensors that say they are on a device, which is as far as the check looks."""
import re

import numpy as np
import pytest


def on_device(t, index=0):
    """t, a host tensor, as a tensor whose `device` is cuda:index"""
    import torch

    class OnDevice(torch.Tensor):
        @property
        def device(self):
            return torch.device("cuda", index)

    return t.as_subclass(OnDevice)


def f32(*shape, index=0):
    import torch

    return on_device(torch.zeros(shape, dtype=torch.float32), index)


def never():
    raise AssertionError("the check let the call through")


def call(stage, x, other, lengths=None, other_lengths=None, out=None):
    from alac.net_amd.mix import _mix
    from alac.net_amd.reverb import _reverb

    if stage == "noise":
        return _mix(never, x, other, never, lengths, other_lengths, out)
    return _reverb(never, x, other, lengths, other_lengths, out)


def refusals(name):
    """(what is wrong, the arguments, the message) for the stage whose companion is called `name`: noise [B, C or 1, T] or
    rir [B, C or 1, K]"""
    import torch

    K = 8 if name == "noise" else 5
    x, other = f32(2, 2, 8), f32(2, 1, K)
    wide = f32(2, 2, 12)
    flat = f32(2 * 2 * 8 + 4)
    a_tensor = "[B, C, T]" if name == "noise" else "[B, C or 1, K]"
    cases = [
        ("x of two dimensions", (f32(2, 8), other), "x must be a float32 device tensor [B, C, T]"),
        ("x without channels", (f32(2, 0, 8), other), "x must be a float32 device tensor [B, C, T]"),
        ("x of float64", (on_device(torch.zeros(2, 2, 8, dtype=torch.float64)), other), "x must be a float32 device tensor [B, C, T]"),
        ("x on the host", (torch.zeros(2, 2, 8), other), "x must be a float32 device tensor [B, C, T]"),
        ("x of another layout", (f32(2, 8, 2).transpose(1, 2), other), "x must be contiguous or the slice [..., :T] of a contiguous tensor"),
        ("no companion", (x, None), f"{name} must be a float32 device tensor {a_tensor}"),
        ("a companion of two dimensions", (x, f32(2, K)), f"{name} must be a float32 device tensor {a_tensor}"),
        ("a companion of float64", (x, on_device(torch.zeros(2, 1, K, dtype=torch.float64))), f"{name} must be a float32 device tensor [B, C, T]"),
        ("a companion on the host", (x, torch.zeros(2, 1, K)), f"{name} must be a float32 device tensor [B, C, T]"),
        ("three channels for two", (x, f32(2, 3, K)), f"{name} must be [2, 2 or 1, {K}], not (2, 3, {K})"),
        ("two channels for one", (f32(2, 1, 8), f32(2, 2, K)), f"{name} must be [2, 1, {K}], not (2, 2, {K})"),
        ("a companion of another batch", (x, f32(3, 1, K)), f"{name} must be [2, 2 or 1, {K}], not (3, 1, {K})"),
        ("a companion of another layout", (x, f32(2, 1, 2 * K)[..., ::2]), f"{name} must be contiguous or the slice [..., :T] of a contiguous tensor"),
        ("a companion on another device", (x, f32(2, 1, K, index=1)), f"x and {name} must be on one device"),
        ("out of another shape", (x, other, None, None, f32(2, 2, 9)), "out must be x itself or a float32 tensor of x's shape, layout and device"),
        ("out of float64", (x, other, None, None, on_device(torch.zeros(2, 2, 8, dtype=torch.float64))),
         "out must be x itself or a float32 tensor of x's shape, layout and device"),
        ("out of another layout", (x, other, None, None, wide[..., :8]), "out must be x itself or a float32 tensor of x's shape, layout and device"),
        ("out on another device", (x, other, None, None, f32(2, 2, 8, index=1)), "out must be x itself or a float32 tensor of x's shape, layout and device"),
        ("out that is no tensor", (x, other, None, None, np.zeros((2, 2, 8), np.float32)), "out must be x itself or a float32 tensor of x's shape, layout and device"),
        ("out that overlaps x", (flat[:32].view(2, 2, 8), other, None, None, flat[4:].view(2, 2, 8)), "out overlaps x without being x"),
        ("a companion that overlaps out", (x, flat[:2 * K].view(2, 1, K), None, None, flat[:32].view(2, 2, 8)), f"{name} overlaps out"),
    ]
    if name == "noise":
        cases.append(("noise of other frames", (x, f32(2, 1, 7)), "noise must be [2, 2 or 1, 8], not (2, 1, 7)"))
    else:
        cases.append(("a response without a frame", (x, f32(2, 1, 0)), "rir must have at least one frame"))
    for k, who in enumerate(("lengths", f"{name}_lengths")):
        both = lambda lens: (x, other) + ((lens, None) if k == 0 else (None, lens))
        cases += [
            (f"three {who}", both([1, 2, 3]), f"{who} must be 2 integers, not (3,) int64"),
            (f"{who} that are no integers", both([1.0, 2.0]), f"{who} must be 2 integers, not (2,) float64"),
            (f"{who} of two dimensions", both(np.zeros((2, 1), np.int64)), f"{who} must be 2 integers, not (2, 1) int64"),
            (f"a tensor of three {who}", both(torch.zeros(3, dtype=torch.int64)), f"{who} must be 2 integers"),
            (f"a floating-point tensor of {who}", both(torch.zeros(2)), f"{who} must be 2 integers"),
            (f"a boolean tensor of {who}", both(torch.zeros(2, dtype=torch.bool)), f"{who} must be 2 integers"),
        ]
    return cases


@pytest.mark.parametrize("name", ["noise", "rir"])
def test_every_refusal_keeps_its_message(name):
    seen = set()
    for what, args, message in refusals(name):
        with pytest.raises(ValueError, match="^" + re.escape(message) + "$"):
            call(name, *args)
        seen.add(message)
    assert len(seen) >= 16


def test_what_the_check_hands_on():
    from alac.net_amd._stageargs import _signal_and_companion

    wide, h = f32(3, 2, 12), f32(3, 1, 20)
    x = wide[..., :8]
    # in place over slices: the plane strides are the wide tensors', out is x, no lengths are no tensors
    for name, other, same in (("noise", h[..., :8], True), ("rir", h[..., :5], False)):
        S, So, out, d_valid, d_other = _signal_and_companion(x, name, other, None, None, x, same_frames=same)
        assert (S, So) == (12, 20) and out is x and d_valid is None and d_other is None
    # one row of one channel has no stride to read: the row's length stands for it; an empty batch passes without a look
    one, empty = f32(1, 1, 8), f32(0, 2, 8)
    S, So, out, _, _ = _signal_and_companion(one, "rir", f32(1, 1, 3), None, None, one, same_frames=False)
    assert (S, So) == (8, 3) and out is one
    assert _signal_and_companion(empty, "noise", f32(0, 1, 8), None, None, empty, same_frames=True)[2] is empty
    # a response may be longer than the crop; its lengths are counted against the batch like the signal's
    assert _signal_and_companion(x, "rir", f32(3, 2, 40), None, None, x, same_frames=False)[:2] == (12, 40)
    with pytest.raises(ValueError, match="^rir_lengths must be 3 integers, not \\(2,\\) int64$"):
        _signal_and_companion(x, "rir", f32(3, 2, 40), None, [50, -1], x, same_frames=False)
