"""fastpath.DeferredStatus on the host, with a stand-in for torch.cuda.Event: which entries an examine() takes and in what order,
that the blocking form never asks an event whether it fired, and that an entry is back in the pools before its decision raises."""
import pytest
import torch

from mygauhuman_amd.fastpath import DeferredStatus


class _Event:
    made = 0

    def __init__(self):
        _Event.made += 1
        self.fired, self.queried, self.waited = False, 0, 0

    def record(self, stream):
        self.fired = False

    def query(self):
        self.queried += 1
        return self.fired

    def synchronize(self):
        self.waited += 1
        self.fired = True


class _Bad(RuntimeError):
    pass


@pytest.fixture
def status(monkeypatch):
    monkeypatch.setattr(torch.cuda, "Event", _Event)
    _Event.made = 0
    seen = []

    def decide(entry, words):
        seen.append((entry.index, entry.tag, words))
        if words[1]:
            raise _Bad(f"entry {entry.index}")
    ds = DeferredStatus(2, decide)
    return ds, seen


def _push(ds, n, bad=()):
    return [ds.push(torch.tensor([10 + k, int(k in bad)], dtype=torch.int32), None, tag=f"t{k}") for k in range(n)]


def test_blocking_examine_goes_by_index_only(status):
    ds, seen = status
    e = _push(ds, 4)
    e[3].event.fired = True                      # a later entry that has fired is NOT taken by the blocking form
    ds.examine(block_older_than=1)
    assert seen == [(0, "t0", [10, 0]), (1, "t1", [11, 0])]
    assert ds.pending == e[2:] and all(x.event.queried == 0 for x in e)
    ds.examine(block_older_than=1, nonblocking=True)   # ... the non-blocking form takes it, and leaves entry 2 waiting
    assert [s[0] for s in seen] == [0, 1, 3] and ds.pending == [e[2]] and e[2].event.waited == 0
    ds.check_all()
    assert [s[0] for s in seen] == [0, 1, 3, 2] and not ds.pending


def test_entry_is_recycled_before_its_decision_raises(status):
    ds, seen = status
    e = _push(ds, 3, bad=(1,))
    with pytest.raises(_Bad, match="entry 1"):
        ds.check_all()
    assert ds.pending == [e[2]]                  # the rest stays for the next call
    assert ds.words() is e[1].words and ds.words() is e[0].words
    ds.check(e[2])
    ds.check(e[2])                               # examined already: nothing happens
    assert [s[0] for s in seen] == [0, 1, 2] and e[2].event.waited == 1
    _push(ds, 3)                                 # warmed up: the three events are reused
    assert _Event.made == 3 and [x.index for x in ds.pending] == [3, 4, 5]
