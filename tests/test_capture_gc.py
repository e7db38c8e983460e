"""Graph captures keep Python's cyclic garbage collector out (optimizers.graphs.no_gc_during_capture): no GPU needed."""
import gc

import pytest

from stabletriton_amd.optimizers.graphs import no_gc_during_capture


class _Cycle:
    freed = 0

    def __init__(self):
        self.me = self

    def __del__(self):
        _Cycle.freed += 1


def test_collects_before_and_holds_the_collector_off():
    assert gc.isenabled()
    _Cycle.freed = 0
    _Cycle()                                          # dead cycle: only the collector frees it
    with no_gc_during_capture():
        assert _Cycle.freed == 1                      # collected before the capture begins
        assert not gc.isenabled()
        _Cycle()
        for _ in range(10000):                        # allocations that would trigger an automatic collection
            [object()]
        assert _Cycle.freed == 1
    assert gc.isenabled()
    gc.collect()
    assert _Cycle.freed == 2


def test_restores_the_collector_after_an_error_and_keeps_it_off_if_it_was():
    with pytest.raises(RuntimeError):
        with no_gc_during_capture():
            raise RuntimeError("capture failed")
    assert gc.isenabled()
    gc.disable()
    try:
        with no_gc_during_capture():
            pass
        assert not gc.isenabled()
    finally:
        gc.enable()
