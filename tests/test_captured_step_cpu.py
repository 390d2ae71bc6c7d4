"""Host decisions of the captured training steps (``nerf/captured.py``) and the fork hook of the table backward
(``network.before_scatter``): CPU tensors of 4 rays, nothing captured, no library call."""
import pytest
import torch

from instance_nerf_amd.nerf import network
from instance_nerf_amd.nerf.captured import GRAPH_ALIGN, BufferSet, HeldCapacity, StepPipeline, graph_key


def test_captured_step_buffer_size_holds_across_small_changes():
    """HeldCapacity.fit: sizes of the captured step's sample buffers - up to GRAPH_ALIGN, kept while the held size
    still fits and is not more than max(2 units, 1/8) too large (every change re-captures the step's graphs)."""
    t = HeldCapacity()
    a = GRAPH_ALIGN
    assert t.fit(1) == a and t.fit(a) == a
    assert t.fit(30 * a - 5) == 30 * a
    assert t.fit(29 * a - 7) == 30 * a               # wandered down a unit: held
    assert t.fit(30 * a - 9) == 30 * a
    assert t.fit(30 * a + 1) == 31 * a               # no longer fits: grows at once
    assert t.fit(28 * a) == 31 * a                   # 3 units under, 1/8 of 28 units = 3.5: held
    assert t.fit(20 * a) == 20 * a                   # the scene emptied: shrinks
    assert t.fit(4 * a) == 4 * a
    assert t.fit(2 * a + 1) == 4 * a                 # small sizes: two units of slack
    assert t.fit(a) == a


def _batch():
    return {"rays_o": torch.zeros(1, 4, 3), "rays_d": torch.ones(1, 4, 3), "masks": torch.zeros(1, 4, dtype=torch.int64),
            "H": 2, "W": 2}


def _pipeline():
    sets = [BufferSet(None, _batch(), torch.zeros(2, dtype=torch.int32)) for _ in range(2)]
    return StepPipeline(None, graph_key(GRAPH_ALIGN, "instance", _batch()), sets, side=None)


def _plan(p, data, next_data=None, global_step=3, interval=16, grid_state=7):
    return p.plan(data, next_data, global_step, interval, grid_state)


def test_a_step_takes_the_prefetched_head_only_for_the_very_tensors_and_grid_it_was_marched_for():
    p, data = _pipeline(), _batch()
    assert p.grid_state is None and p.captures == 0 and p.graphs == {} and p.turn == 0
    assert _plan(p, data)[0] is True                                 # first step
    # the previous step looked ahead into this very rays_o, through grid generation 7
    p.primed, p.expect, p.grid_state = True, data["rays_o"], 7
    assert _plan(p, data)[0] is False
    other = dict(data, rays_o=data["rays_o"].clone())
    assert torch.equal(other["rays_o"], data["rays_o"]) and _plan(p, other)[0] is True       # equal values, another object
    assert _plan(p, data, grid_state=8)[0] is True                   # an occupancy update in between
    p.primed, p.expect = False, None                                 # the previous step did not look ahead
    assert _plan(p, data)[0] is True
    p.expect = data["rays_o"]                                        # ... whatever was expected once
    assert _plan(p, data)[0] is True
    assert p.primed is False and p.expect is data["rays_o"] and p.grid_state == 7 and p.turn == 0     # plan changes nothing


def test_a_step_looks_ahead_only_into_a_batch_of_the_other_sets_layout_and_never_across_an_update():
    p, data = _pipeline(), _batch()
    assert _plan(p, data, None)[1] is False                          # no next batch
    assert _plan(p, data, _batch())[1] is True
    assert _plan(p, data, _batch(), global_step=32)[1] is False      # the next call starts with an occupancy update
    assert _plan(p, data, _batch(), global_step=33)[1] is True
    lacking = _batch()
    del lacking["masks"]
    assert _plan(p, data, lacking)[1] is False                       # a tensor of the static batch is missing
    assert _plan(p, data, dict(_batch(), masks=3))[1] is False       # ... or is no tensor
    assert _plan(p, data, dict(_batch(), rays_d=torch.ones(1, 5, 3)))[1] is False            # another shape
    assert _plan(p, data, dict(_batch(), masks=torch.zeros(1, 4, dtype=torch.int32)))[1] is False    # another dtype
    assert _plan(p, data, dict(_batch(), extra=torch.zeros(9)))[1] is True                   # more than the static batch: fine
    # it is the OTHER set's layout that counts: the look-ahead fills the set the next step reads
    p.sets[1].static["rays_d"] = torch.ones(1, 5, 3)
    assert _plan(p, data, _batch())[1] is False
    p.turn = 1
    assert _plan(p, data, _batch())[1] is True
    assert _plan(p, data, _batch()) == (True, True)                  # the key of the graph: (turn, prime, ahead)


def test_the_graph_key_is_the_layout_of_a_batch_not_its_values():
    a, b = _batch(), _batch()
    b["rays_o"] = b["rays_o"] + 1
    b["H"] = 4                                                       # not a tensor
    assert graph_key(GRAPH_ALIGN, "instance", a) == graph_key(GRAPH_ALIGN, "instance", b)
    assert graph_key(GRAPH_ALIGN, "instance", a) != graph_key(GRAPH_ALIGN, "instance", dict(a, rays_o=torch.zeros(1, 5, 3)))
    assert graph_key(GRAPH_ALIGN, "instance", a) != graph_key(2 * GRAPH_ALIGN, "instance", a)
    assert graph_key(GRAPH_ALIGN, "instance", a) != graph_key(GRAPH_ALIGN, "nerf", a)


def test_the_fork_hook_fires_once_and_never_outlives_its_block():
    calls = []
    with network.before_scatter(lambda: calls.append("a")) as fork:
        assert not fork.fired and calls == []
        network.before_scatter.take()                                # what _table_backward does before its first scatter
        assert fork.fired and calls == ["a"]
        network.before_scatter.take()                                # a second table backward in the same block
        assert calls == ["a"]
    assert network.before_scatter.pending is None

    with network.before_scatter(lambda: calls.append("b")) as fork:
        pass                                                         # no fused table backward ran
    assert not fork.fired and network.before_scatter.pending is None
    network.before_scatter.take()
    assert calls == ["a"]

    with pytest.raises(ZeroDivisionError):
        with network.before_scatter(lambda: calls.append("c")):
            1 / 0                                                    # a backward that raises before the table's turn
    assert network.before_scatter.pending is None
    network.before_scatter.take()
    assert calls == ["a"]


def test_a_second_fork_hook_is_refused_while_one_is_pending():
    calls = []
    with network.before_scatter(lambda: calls.append("first")) as first:
        with pytest.raises(RuntimeError):
            with network.before_scatter(lambda: calls.append("second")):
                pass
        assert network.before_scatter.pending is first and not first.fired
        network.before_scatter.take()
        assert calls == ["first"]
        with network.before_scatter(lambda: calls.append("third")) as third:     # the first has fired: the place is free
            network.before_scatter.take()
        assert third.fired
    assert calls == ["first", "third"] and network.before_scatter.pending is None
