"""The validity rules of a prefetched training head (``renderer.MarchedHead``) and the ``step_counter`` slot bookkeeping
around it: host logic only - CPU tensors of 4 rays, no library call."""
import torch

from instance_nerf_amd.nerf.renderer import MarchedHead


def _head(labels=None, **kw):
    ro, rd = torch.zeros(1, 4, 3), torch.ones(1, 4, 3)
    return ro, rd, MarchedHead(ro, rd, labels, n_rays=4, grid_state=7, **kw)


def test_a_head_serves_the_tensors_and_labels_it_was_marched_for_and_no_others():
    ro, rd, h = _head()
    assert h.marched_for(ro, rd, None)                               # marched without labels, asked without
    assert not h.marched_for(ro.clone(), rd, None) and not h.marched_for(ro, rd.clone(), None)    # equal values, other objects
    assert not h.marched_for(rd, ro, None)
    labels = torch.tensor([[0, -1, 2, 1]])
    assert not h.marched_for(ro, rd, labels)                         # marched without labels, asked with
    ro, rd, h = _head(labels)
    assert h.marched_for(ro, rd, labels)
    assert not h.marched_for(ro, rd, labels.clone())                 # another label tensor
    assert not h.marched_for(ro, rd, None)                           # marched with labels, asked without


def test_a_head_fits_a_training_render_of_its_ray_count_through_its_grid_generation():
    _, _, h = _head()
    assert h.fits(True, 4, 7)
    assert not h.fits(True, 5, 7)                                    # another ray count
    assert not h.fits(True, 4, 8)                                    # the occupancy grid was updated since
    assert not h.fits(False, 4, 7)                                   # eval mode


def test_pre_shaded_outputs_go_with_the_threshold_and_scale_they_were_computed_for():
    shaded = tuple(torch.zeros(4) for _ in range(5))
    _, _, h = _head(shaded=shaded, T_thresh=1e-4, density_scale=1)
    assert h.shaded_for(1e-4, 1) is shaded and h.shaded_for(1e-4, 1.0) is shaded
    assert h.shaded_for(1e-3, 1) is None
    assert h.shaded_for(1e-4, 2.0) is None
    _, _, bare = _head()
    assert bare.shaded_for(1e-4, 1) is None                          # nothing was shaded ahead


def test_the_capture_variant_waits_on_nothing_and_is_valid_for_the_generation_given():
    class Recorded:                     # stands for an event on a side stream: waiting for it would need a device
        pass
    shaded = tuple(torch.zeros(4) for _ in range(5))
    buffers = {k: torch.zeros(4) for k in ("nears", "fars", "xyzs", "dirs", "deltas", "rays", "counter")}
    labels = torch.tensor([[0, -1, 2, 1]])
    ro, rd, h = _head(labels, shaded=shaded, T_thresh=1e-3, density_scale=2, done=Recorded(), side=Recorded(), **buffers)
    c = h.ordered_here(9)
    c.wait()                            # no event, so no stream is asked for either
    assert c.done is None and c.fits(True, 4, 9) and not c.fits(True, 4, 7)
    assert h.fits(True, 4, 7) and h.done is not None                 # the original is as it was
    assert c.marched_for(ro, rd, labels) and c.shaded_for(1e-3, 2) is shaded
    assert all(getattr(c, k) is v for k, v in buffers.items())
    assert not c.slot_taken


def test_counter_slots_are_taken_in_turn_and_handed_back_only_while_they_are_the_newest():
    """The rule of test_gpu_parity.py::test_dropping_a_prefetched_march_never_steps_over_a_later_slot, on host integers."""
    from instance_nerf_amd.nerf import NeRFNetwork
    net = NeRFNetwork(cuda_ray=True, num_instances=0, min_near=0.05).train()

    def take():
        index, row = net._take_counter_slot()
        assert row.data_ptr() == net.step_counter[index].data_ptr() and row.shape == (2,)
        return MarchedHead(None, None, None, n_rays=4, grid_state=0, counter=row, slot_taken=True, slot_index=index)
    a = take()
    assert a.slot_index == 0 and net.local_step == 1
    net.drop_ahead(a)                                   # still the newest slot: handed back
    assert net.local_step == 0 and not a.slot_taken
    net.drop_ahead(a)                                   # only once
    assert net.local_step == 0
    a = take()                                          # slot 0 again
    assert a.slot_index == 0
    assert net._take_counter_slot()[0] == 1             # another march takes slot 1
    net.drop_ahead(a)                                   # NOT the newest slot any more: nothing moves
    assert net.local_step == 2 and not a.slot_taken
    assert net._take_counter_slot()[0] == 2
    net.local_step = 16                                 # the ring wraps
    b = take()
    assert b.slot_index == 0 and net.local_step == 17
    net.drop_ahead(b)
    assert net.local_step == 16
    own = MarchedHead(None, None, None, n_rays=4, grid_state=0, counter=torch.zeros(2, dtype=torch.int32))
    net.drop_ahead(own)                                 # a caller-owned counter took no slot
    net.drop_ahead(None)
    assert net.local_step == 16
