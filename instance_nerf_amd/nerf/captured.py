"""The training step captured as a hipGraph: the one-stream ``CapturedStep`` (``Trainer(use_graph=True)``) and the
two-stream ``StepPipeline`` (``use_graph=True, look_ahead=True``), with the buffer-size rule and the host bookkeeping
they share.  ``Trainer.train_one_step`` chooses the mode and keeps one of them per batch layout; both call back into the
trainer they were built for (``train_step``, ``_lr_step``, ``_skip_labels``, ``_pipe_args``, optimiser, model, EMA)."""
import ctypes

import torch

from .. import _lib
from . import network as _network

GRAPH_ALIGN = 16384        # buffer sizes are rounded up to this many samples so that a graph survives the
                           # small changes of mean_count at every occupancy update


class HeldCapacity:
    """Sample-buffer size of the captured step for a measured ``mean_count``: rounded up to GRAPH_ALIGN, and the size
    already captured for is kept while it still holds the batch and is at most max(2 units, 1/8) too large - the
    16-step mean of a converged scene wanders by a few thousand samples, and every change of the size is a new set
    of graphs (tools/pipeline_convergence_probe.py: without the hold, 84 captures in 31 updates)."""

    def __init__(self):
        self.held = 0

    def fit(self, mean_count):
        a = GRAPH_ALIGN
        need = (mean_count + a - 1) // a * a
        held = self.held
        if need <= held <= need + max(2 * a, need // 8):
            need = held
        self.held = need
        return need


def copy_tensors(pairs):
    """[(dst, src)] device tensors of equal size: ONE launch for up to 8 of them (``inr_copy_multi``) when they are
    contiguous GPU tensors of the same dtype with 4-byte-multiple sizes, ``dst.copy_(src)`` otherwise."""
    fast = [(d, s) for d, s in pairs if d.is_cuda and s.is_cuda and d.dtype == s.dtype and d.is_contiguous()
            and s.is_contiguous() and d.numel() == s.numel() and (d.numel() * d.element_size()) % 4 == 0
            and d.device == s.device and d.data_ptr() % 4 == 0 and s.data_ptr() % 4 == 0]
    for d, s in pairs:
        if not any(d is f[0] for f in fast):
            d.copy_(s, non_blocking=True)
    lib = _lib.load()
    for i in range(0, len(fast), 8):
        chunk = fast[i:i + 8]
        n = len(chunk)
        _lib.check(lib.inr_copy_multi(n, (ctypes.c_void_p * n)(*[d.data_ptr() for d, _ in chunk]),
                                      (ctypes.c_void_p * n)(*[s.data_ptr() for _, s in chunk]),
                                      (ctypes.c_int64 * n)(*[d.numel() * d.element_size() for d, _ in chunk]),
                                      _lib.stream_ptr()), "copy_multi")


def graph_key(mean_count, stage, data):
    """What a captured step is valid for: the buffer size, the stage and the batch's tensor shapes - not its values."""
    return (mean_count, stage) + tuple((k, tuple(v.shape)) for k, v in sorted(data.items()) if torch.is_tensor(v))


def _static_copy(data):
    return {k: (v.clone() if torch.is_tensor(v) else v) for k, v in data.items()}


def _prepare_capture(opt, device):
    """Moments, fixed-point gradient state and the hyper-parameter tensor must exist BEFORE a capture (an allocation
    + zero fill inside it would be replayed every step)."""
    for g in opt.param_groups:
        for p in g["params"]:
            if p.requires_grad:
                opt._moments(p)
                if getattr(p, "_is_hash_table", False):
                    _network.fx_state(p)
                    if _network.fx_bits() == 64:
                        _network.fx_acc64(p)
    opt.hyper_tensor(device)


def _replay_step(tr, graph, written):
    """Replays one captured step with the host bookkeeping around it.  ``written``: the counter the graph's march
    wrote, copied to the renderer's ``step_counter`` slot of this step; None when the total is there already."""
    m = tr.model
    tr._lr_step()
    tr.optimizer.refresh_hyper()
    graph.replay()
    if written is not None:
        m.step_counter[m.local_step % 16].copy_(written)
    m.local_step += 1
    tr.optimizer.bump_versions()
    if tr.ema is not None:
        tr.ema.update()


class CapturedStep:
    """The whole step - march, fields, compositing, loss, backward, Adam - as one hipGraph on one stream."""
    __slots__ = ("trainer", "graph", "static", "loss", "slot", "key")

    def __init__(self, trainer, graph, static, loss, slot, key):
        self.trainer = trainer
        self.graph, self.loss = graph, loss
        self.static = static              # the batch the graph reads: every replay copies its inputs here
        self.slot = slot                  # the renderer's step_counter slot the graph's march always writes
        self.key = key

    @classmethod
    def capture(cls, tr, data):
        m = tr.model
        static = _static_copy(data)
        slot = m.local_step % 16
        _prepare_capture(tr.optimizer, tr.device)
        tr.optimizer.zero_grad()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            _, _, loss = tr.train_step(static)
            loss.backward()
            tr.optimizer.step_captured()
        m.local_step -= 1                       # the capture pass launched nothing; undo its bookkeeping
        return cls(tr, g, static, loss, slot, graph_key(m.mean_count, tr.stage, data))

    def replay(self, data):
        m = self.trainer.model
        copy_tensors([(self.static[k], v) for k, v in data.items() if torch.is_tensor(v)])
        # the graph always writes the slot it was captured with
        _replay_step(self.trainer, self.graph, m.step_counter[self.slot] if m.local_step % 16 != self.slot else None)
        return self.loss.detach()


class BufferSet:
    """One of the pipeline's two persistent batches: the marcher's buffers, the static inputs a graph reads, the
    counter its march writes and the head marched into them by the newest capture (a ``MarchedHead``, or None)."""
    __slots__ = ("bufs", "static", "counter", "marched")

    def __init__(self, bufs, static, counter, marched=None):
        self.bufs, self.static, self.counter, self.marched = bufs, static, counter, marched


class StepPipeline:
    """The captured two-stream step.  The step is bound by the table-gradient scatter (memory-side atomic unit; the CUs
    idle for most of it) and by the host (0.6-0.85 ms to enqueue 0.83 ms of kernels; a second queue costs the runtime
    ~0.3 ms more per step, profiles/r03_NOTES.txt 16).  Both at once: ONE hipGraph per step holds the step's own
    launches on the capture stream and, forked off right before the scatter, the parameter-independent head of the NEXT
    batch on a second stream - ray/box test, march and, in the instance stage, the frozen NeRF's forward and the weight
    compositing (``NeRFRenderer.march_ahead(shade=True)``) - joined again before the graph ends.  Two persistent buffer
    sets alternate (step i reads set A and fills B, step i+1 reads B and fills A), so there is one graph per
    ``(turn, prime, ahead)``: the set, does the step compute its own head, does it look ahead.  The first step after an
    occupancy update computes its own head (the grid changed), the last one before an update does not look ahead
    (``plan``)."""
    __slots__ = ("trainer", "key", "sets", "graphs", "turn", "primed", "expect", "grid_state", "side", "captures")

    def __init__(self, trainer, key, sets, side, captures=0):
        self.trainer, self.key, self.sets, self.side = trainer, key, sets, side
        self.graphs = {}                  # (turn, prime, ahead) -> (graph, loss)
        self.turn = 0                     # the set this step reads
        # the previous step looked ahead (primed) into the batch whose rays_o is `expect`, through the occupancy grid of
        # generation `grid_state` (the renderer's iter_density)
        self.primed, self.expect, self.grid_state = False, None, None
        self.captures = captures          # graphs captured so far, carried over when the buffers are re-allocated

    @classmethod
    def allocate(cls, tr, data, captures=0):
        from .. import raymarching
        m, dev = tr.model, data["rays_o"].device
        N = data["rays_o"].numel() // 3
        M_al = raymarching.sample_capacity(m.mean_count)
        shade = tr.stage == "instance" and tr.shade_ahead and m.shade_ahead_applies()
        sets = [BufferSet(raymarching.march_train_buffers(N, M_al, dev, shade=shade), _static_copy(data),
                          torch.zeros(2, dtype=torch.int32, device=dev)) for _ in range(2)]
        _prepare_capture(tr.optimizer, dev)
        return cls(tr, graph_key(m.mean_count, tr.stage, data), sets, torch.cuda.Stream(device=dev), captures)

    def plan(self, data, next_data, global_step, update_extra_interval, grid_state):
        """-> (prime, ahead): does the step compute its own head, does it look ahead.  No side effect, no GPU call."""
        # the prefetched head is this batch's only if it was marched for these tensors through the occupancy grid as it is
        # NOW (an update between the two steps - the trainer's own never falls there, a caller's may - bumps iter_density)
        prime = not (self.primed and self.expect is data["rays_o"] and self.grid_state == grid_state)
        # no look-ahead across an occupancy update (global_step is already advanced: the next call starts with one
        # when it is a multiple of the interval), nor into a batch of another shape
        ahead = (next_data is not None and global_step % update_extra_interval != 0
                 and all(torch.is_tensor(next_data.get(k)) and next_data[k].shape == v.shape and next_data[k].dtype == v.dtype
                         for k, v in self.sets[self.turn ^ 1].static.items() if torch.is_tensor(v)))
        return prime, ahead

    def capture(self, turn, prime, ahead):
        tr = self.trainer
        m = tr.model
        S, Nx = self.sets[turn], self.sets[turn ^ 1]
        if not prime and S.marched is None:
            raise RuntimeError("pipeline: a step that consumes a prefetched head was asked for before any prefetch")
        tr.optimizer.zero_grad()
        torch.cuda.synchronize()
        step0 = m.local_step
        g = torch.cuda.CUDAGraph()
        try:
            loss = self._capture_body(g, S, Nx, prime, ahead, tr._pipe_args())
        finally:
            tr._ahead = None
            m.local_step = step0                # the capture pass launched nothing; undo its bookkeeping
        G = self.graphs[(turn, prime, ahead)] = (g, loss)
        self.captures += 1
        return G

    def _capture_body(self, g, S, Nx, prime, ahead, args):
        from .. import raymarching
        tr, side = self.trainer, self.side
        m = tr.model
        with torch.cuda.graph(g):
            if prime:
                S.marched = m.march_ahead(S.static["rays_o"], S.static["rays_d"], stream=None, bufs=S.bufs,
                                          counter=S.counter, skip_labels=tr._skip_labels(S.static), **args)
                if S.marched is None:
                    raise RuntimeError("pipeline: march_ahead refused the batch (not the steady state / staged marcher)")
            # same graph or an earlier replay on the same stream: ordered already
            # (the head may come from an earlier capture; whether the buffers' CONTENT is current is step()'s business
            # at every replay, so the renderer's own staleness check must not refuse it while the graph is captured)
            tr._ahead = S.marched.ordered_here(getattr(m, "iter_density", 0))

            def hook():
                Nx.marched = m.march_ahead(Nx.static["rays_o"], Nx.static["rays_d"], stream=side, bufs=Nx.bufs,
                                           counter=Nx.counter, skip_labels=tr._skip_labels(Nx.static), **args)
            if ahead and tr.pipe_fork == "start":
                hook()                               # fork right away: beside the whole step
            _, _, loss = tr.train_step(S.static)
            if tr._ahead is not None:
                raise RuntimeError("pipeline: the render did not take the prefetched head")
            unit = raymarching.unit_gradient(loss.device)
            if ahead and tr.pipe_fork != "start":
                with _network.before_scatter(hook) as fork:      # fork from inside the backward, right before the scatter
                    loss.backward(gradient=unit)
                if not fork.fired:
                    hook()                           # no fused table backward ran (composable path): fork here
            else:
                loss.backward(gradient=unit)
            tr.optimizer.step_captured()
            if ahead:
                torch.cuda.current_stream().wait_stream(side)        # join: the graph ends with both branches done
        return loss

    def step(self, data, next_data):
        tr = self.trainer
        m = tr.model
        t = self.turn
        S, Nx = self.sets[t], self.sets[t ^ 1]
        grid_state = getattr(m, "iter_density", 0)
        prime, ahead = self.plan(data, next_data, tr.global_step, tr.update_extra_interval, grid_state)
        pairs = []
        if prime:
            pairs += [(S.static[k], v) for k, v in data.items() if torch.is_tensor(v)]
        if ahead:
            pairs += [(Nx.static[k], v) for k, v in next_data.items() if torch.is_tensor(v)]
        if not prime:
            # the march of THIS batch ran in the previous replay, into the set's own counter: it goes to the renderer's
            # slot together with the inputs (one launch); a step that marches itself copies after its replay
            pairs.append((m.step_counter[m.local_step % 16], S.counter))
        graph, loss = self.graphs.get((t, prime, ahead)) or self.capture(t, prime, ahead)
        copy_tensors(pairs)
        _replay_step(tr, graph, S.counter if prime else None)
        m.last_counter = S.counter
        self.primed, self.expect = ahead, (next_data["rays_o"] if ahead else None)
        self.grid_state = grid_state
        self.turn = t ^ 1
        return loss.detach()
