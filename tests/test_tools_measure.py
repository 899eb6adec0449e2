"""tools/_measure.py, the one harness behind the benchmark tools.  CPU: event_ms and wall_ms over a stand-in for torch whose
events, synchronizes and calls append to a log and whose calls move a clock -- the whole log and every kept value are compared
with what the module's docstring promises; stats, the two verdicts and make_file by hand.  GPU: two converted tools run once in
a child process each, and their documents keep the key tree the tools have always printed."""
import json
import math
import os
import subprocess
import sys
import types
import weakref

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import _measure  # noqa: E402

STREAM = "the stream"


class FakeTorch:
    """cuda.Event, cuda.synchronize and record append to `log`; a way's k-th call appends too and moves the clock by base + k ms"""

    def __init__(self):
        self.log, self.now, self.calls = [], 0.0, {}
        fake = self

        class Event:
            def __init__(self, enable_timing=False):
                assert enable_timing

            def record(self, stream):
                self.t = fake.now
                fake.log.append(("record", stream))

            def synchronize(self):
                fake.log.append(("event.synchronize",))

            def elapsed_time(self, end):
                return end.t - self.t

        self.cuda = types.SimpleNamespace(Event=Event, synchronize=lambda: self.log.append(("synchronize",)))

    def way(self, name, base):
        def fn(*args):
            k = self.calls.get(name, 0)
            self.calls[name] = k + 1
            self.now += base + k
            self.log.append(("call", name) + args)

        return fn

    def before(self, name):
        return lambda *args: self.log.append(("before", name) + args)


def repetition(way, reps, before=False):
    """What one repetition of event_ms leaves in the log"""
    return ([("before", way)] if before else []) + [("synchronize",), ("record", STREAM)] + [("call", way)] * reps \
        + [("record", STREAM), ("event.synchronize",)]


def kept_ms(base, steps, warmup, reps):
    """Repetition r makes the calls k = r reps .. r reps + reps - 1 of base + k ms each: their mean, for every r >= warmup"""
    return [base + r * reps + (reps - 1) / 2 for r in range(warmup, warmup + steps)]


def test_event_ms_in_sequence_runs_a_way_to_its_end_before_the_next():
    fake = FakeTorch()
    steps, warmup, reps = 3, 2, 4
    ms = _measure.event_ms(fake, STREAM, {"A": fake.way("A", 10.0), "B": fake.way("B", 500.0)}, steps, warmup, reps, alternate=False)
    assert fake.log == repetition("A", reps) * (steps + warmup) + repetition("B", reps) * (steps + warmup)
    called = [e[1] for e in fake.log if e[0] == "call"]
    assert called == ["A"] * (reps * (steps + warmup)) + ["B"] * (reps * (steps + warmup))
    assert list(ms) == ["A", "B"]
    assert ms["A"] == kept_ms(10.0, steps, warmup, reps) and ms["B"] == kept_ms(500.0, steps, warmup, reps)
    assert len(ms["A"]) == len(ms["B"]) == steps


def test_event_ms_alternating_takes_turns_inside_every_repetition():
    fake = FakeTorch()
    steps, warmup, reps = 3, 1, 2
    ms = _measure.event_ms(fake, STREAM, {"A": fake.way("A", 10.0), "B": fake.way("B", 500.0)}, steps, warmup, reps, alternate=True)
    assert fake.log == (repetition("A", reps) + repetition("B", reps)) * (steps + warmup)
    firsts = [fake.log[i + 1][1] for i, e in enumerate(fake.log) if e == ("record", STREAM) and fake.log[i + 1][0] == "call"]
    assert firsts == ["A", "B"] * (steps + warmup)
    assert ms == {"A": kept_ms(10.0, steps, warmup, reps), "B": kept_ms(500.0, steps, warmup, reps)}


@pytest.mark.parametrize("reps", [1, 5])
def test_event_ms_has_exactly_reps_calls_between_two_records(reps):
    fake = FakeTorch()
    _measure.event_ms(fake, STREAM, {"A": fake.way("A", 1.0)}, 2, 1, reps, alternate=False)
    at = [i for i, e in enumerate(fake.log) if e[0] == "record"]
    assert len(at) == 2 * 3
    for first, second in zip(at[0::2], at[1::2]):
        assert fake.log[first + 1:second] == [("call", "A")] * reps


def test_event_ms_takes_a_count_per_way():
    fake = FakeTorch()
    ms = _measure.event_ms(fake, STREAM, {"A": fake.way("A", 10.0), "B": fake.way("B", 500.0)}, 2, 1, {"A": 3, "B": 1}, alternate=True)
    assert fake.log == (repetition("A", 3) + repetition("B", 1)) * 3
    assert ms == {"A": kept_ms(10.0, 2, 1, 3), "B": kept_ms(500.0, 2, 1, 1)}


@pytest.mark.parametrize("alternate", [False, True])
def test_event_ms_before_runs_in_front_of_the_synchronize_and_only_for_its_way(alternate):
    fake = FakeTorch()
    steps, warmup, reps = 2, 1, 2
    ms = _measure.event_ms(fake, STREAM, {"A": fake.way("A", 10.0), "B": fake.way("B", 500.0)}, steps, warmup, reps, alternate=alternate,
                           before={"B": fake.before("B")})
    a, b = repetition("A", reps), repetition("B", reps, before=True)
    assert b[:3] == [("before", "B"), ("synchronize",), ("record", STREAM)]             # in front of the synchronize, outside the events
    assert fake.log == ((a + b) * (steps + warmup) if alternate else a * (steps + warmup) + b * (steps + warmup))
    assert ms == {"A": kept_ms(10.0, steps, warmup, reps), "B": kept_ms(500.0, steps, warmup, reps)}      # and it costs no time


def test_wall_ms_alternates_hands_over_the_step_and_times_only_the_call(monkeypatch):
    fake = FakeTorch()
    monkeypatch.setattr(_measure, "time", types.SimpleNamespace(perf_counter=lambda: fake.now * 1e-3))
    steps, warmup = 3, 2
    results = []

    class Result:
        pass

    def returning(fn):
        def run(i):
            assert all(r() is None for r in results), "an earlier result is still alive"
            fn(i)
            out = Result()
            results.append(weakref.ref(out))
            return out

        return run

    ways = {"A": returning(fake.way("A", 10.0)), "B": returning(fake.way("B", 500.0))}
    ms = _measure.wall_ms(fake, ways, steps, warmup)
    assert fake.log == [e for i in range(steps + warmup) for way in ("A", "B") for e in (("synchronize",), ("call", way, i), ("synchronize",))]
    assert [e[2] for e in fake.log if e[:2] == ("call", "A")] == [0, 1, 2, 3, 4]
    assert ms == {"A": pytest.approx([10.0 + i for i in range(warmup, warmup + steps)]),
                  "B": pytest.approx([500.0 + i for i in range(warmup, warmup + steps)])}
    assert len(ms["A"]) == len(ms["B"]) == steps and len(results) == 2 * (steps + warmup)


def test_wall_ms_before_gets_the_step_in_front_of_every_ways_synchronize(monkeypatch):
    fake = FakeTorch()
    monkeypatch.setattr(_measure, "time", types.SimpleNamespace(perf_counter=lambda: fake.now * 1e-3))
    ms = _measure.wall_ms(fake, {"A": fake.way("A", 10.0), "B": fake.way("B", 500.0)}, 1, 1, before=fake.before("all"))
    assert fake.log == [e for i in range(2) for way in ("A", "B")
                        for e in (("before", "all", i), ("synchronize",), ("call", way, i), ("synchronize",))]
    assert ms == {"A": pytest.approx([11.0]), "B": pytest.approx([501.0])}


def test_stats_by_hand():
    # sorted: 1.00004, 2.00006, 3.00007.  p10 lies 0.2 of the way from the first to the second, p90 0.8 from the second to the third
    assert _measure.stats([3.00007, 1.00004, 2.00006]) == {"median": 2.0001, "p10": 1.2, "p90": 2.8001}
    assert _measure.stats(list(range(1, 12))) == {"median": 6.0, "p10": 2.0, "p90": 10.0}
    assert _measure.stats([0.12345678]) == {"median": 0.1235, "p10": 0.1235, "p90": 0.1235}


def test_verdicts_at_their_edges():
    parent = {"median": 1.5, "p10": 1.0, "p90": 2.0}
    at = lambda median: {"median": median, "p10": median - 0.3, "p90": median + 0.3}
    assert [_measure.inside(parent, at(m)) for m in (0.9999, 1.0, 2.0, 2.0001)] == [False, True, True, False]
    assert [_measure.not_above(parent, at(m)) for m in (0.9999, 1.0, 2.0, 2.0001)] == [True, True, True, False]
    assert all(type(f(parent, at(1.5))) is bool for f in (_measure.inside, _measure.not_above))


@pytest.mark.parametrize("rate", [44100, 48000])
def test_make_file_parses_to_its_frames_at_its_rate(synth, rate):
    from alac.net_amd import container

    data = _measure.make_file(synth, 2 * 4096 + 5, 7, rate)
    t = container.packet_table(data)
    assert list(t["durations"]) == [4096, 4096, 5] and t["num_samples"] == 2 * 4096 + 5
    assert t["sample_rate"] == rate and t["num_channels"] == 2 and t["sample_size"] == 16
    assert (data == _measure.make_file(synth, 2 * 4096 + 5, 7)) == (rate == 44100)        # (44100 is the default)


# ---- two converted tools, once each, on the GPU ---------------------------------------------------------------------------------

MS = {"median": None, "p10": None, "p90": None}
NORMALIZE = {"command": None, "steps": None, "warmup": None, "reps": None,
             "results": [{"case": None, "agrees_with_torch": None,
                          "ms_per_call_events_around_reps_calls": {"normalize": MS, "torch_composition": MS},
                          "normalize_median_below_torch_p10": None}] * 4}
MIX = {"command": None, "steps": None, "warmup": None, "reps": None,
       "calls": [{"shape": [None, None, None], "agrees_with_torch": None,
                  "ms_per_call_events_around_reps_calls": {"mix_call": MS, "torch_composition": MS},
                  "mix_call_median_below_torch_median": None, "least_bytes": None, "mix_call_gb_per_s_of_least_bytes": None}] * 2,
       "step": {"step": None, "wall_ms": {"mix": MS, "without": MS}}}


def key_tree(x):
    if isinstance(x, dict):
        return {k: key_tree(v) for k, v in x.items()}
    return [key_tree(v) for v in x] if isinstance(x, list) else None


def times(x):
    """Every {median, p10, p90} block below x"""
    if isinstance(x, dict):
        return [x] if list(x) == list(MS) else [t for v in x.values() for t in times(v)]
    return [t for v in x for t in times(v)] if isinstance(x, list) else []


@pytest.mark.gpu
@pytest.mark.parametrize("tool,more,tree,entries,blocks", [("bench_normalize.py", [], NORMALIZE, "results", 4 * 2),
                                                          ("bench_mix.py", ["--files", "2", "--seconds", "3"], MIX, "calls", 2 * 2 + 2)],
                         ids=["events_in_sequence", "events_and_wall_step"])
def test_a_converted_tool_prints_the_document_it_always_printed(tmp_path, tool, more, tree, entries, blocks):
    out = tmp_path / "doc.json"
    args = more + ["--steps", "2", "--warmup", "1", "--reps", "1", "--out", str(out)]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", tool)] + args, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    doc = json.loads(out.read_text())
    assert json.loads(r.stdout) == doc                                                   # printed and written: one document
    assert json.dumps(key_tree(doc)) == json.dumps(tree)                                 # (as text: the order of the keys too)
    assert doc["command"] == f"python tools/{tool} " + " ".join(args) and (doc["steps"], doc["warmup"], doc["reps"]) == (2, 1, 1)
    assert all(e["agrees_with_torch"] is True for e in doc[entries])
    found = times(doc)
    assert len(found) == blocks
    for t in found:
        assert all(type(v) is float and math.isfinite(v) and v > 0 for v in t.values()), t
