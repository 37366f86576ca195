"""tools/abtime.py, the family benchmarks' A/B protocol, with a fake stream and a fake timer: no GPU, no torch."""
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "tools"))
import abtime


class FakeStream:
    def __init__(self, log):
        self.log = log

    def synchronize(self):
        self.log.append("sync")


def test_alternate_warms_every_candidate_then_alternates_in_one_order():
    log = []
    names = ["fused", "composed", "by hand"]
    calls = {k: (lambda k=k: log.append(("call", k))) for k in names}
    stream = FakeStream(log)

    def timer(s, call, reps):
        assert s is stream
        before = len(log)
        call()  # which candidate: its own record
        kind, k = log.pop()
        assert kind == "call" and len(log) == before
        log.append(("timed", k, reps))
        return float(len(log))

    times = abtime.alternate(stream, calls, warmup=3, rounds=5, reps={"fused": 10, "composed": 10, "by hand": 2}, timer=timer)
    warm = [("call", k) for k in names for _ in range(3)]
    assert log[:9] == warm  # each candidate's warm-ups, nothing timed among them
    assert log[9] == "sync"  # and finished before the first timed round
    rounds = log[10:]
    one_round = [("timed", "fused", 10), ("timed", "composed", 10), ("timed", "by hand", 2)]
    assert rounds == one_round * 5  # the same order in every round
    assert list(times) == names and all(len(t) == 5 for t in times.values())
    assert times["fused"] == [11.0, 14.0, 17.0, 20.0, 23.0]  # what the timer returned, per candidate, in round order

    log.clear()
    assert abtime.alternate(stream, calls, warmup=0, rounds=2, reps=7, timer=timer) == {"fused": [2.0, 5.0], "composed": [3.0, 6.0], "by hand": [4.0, 7.0]}
    assert log[0] == "sync" and all(e[2] == 7 for e in log[1:])


def test_cell_is_median_min_max():
    assert abtime.cell([3, 1, 2]) == "2.000 ms [1.000 .. 3.000]"
    assert abtime.cell([0.5]) == "0.500 ms [0.500 .. 0.500]"
