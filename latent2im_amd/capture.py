"""The walk-training step as a hipGraph (BASELINE config 5: "hipGraph-captured step").

Everything between "z and alpha are on the device" and "the walk gradient is complete" is static-shaped GPU work issued from
Python one launch at a time (~300 conv launches + ~500 small kernels per step).  ``CapturedStep`` records that region ONCE with
``torch.cuda.graph`` (HIP stream capture -> hipGraphInstantiate) and replays it with a single ``hipGraphLaunch`` per step:

    z, alpha (static device buffers, refilled by an async copy before each replay)
      -> style MLP -> synthesis (x0) -> regressor -> epsilon (device-side: no ``.item()``, no host read of alpha_org)
      -> walk -> synthesis (x1) -> D / VGG / regressor losses on their three streams (forked from and joined to the captured
         stream) -> backward into ``walk.grad``

``CapturedZStep`` is the same for BASELINE config 1, the PGGAN graph's walk in z (pggan.walk_forward_backward): one stream, no noise.
``record`` is the one place that records a step; the inversion's iteration (invert._Replay) goes through it too.

The all-reduce of the walk gradient (RCCL) and the Adam update (WalkGraph.walk_update) stay OUTSIDE the graph, in the order optimizeParametersAll
runs them: a handful of tiny launches, and the captured region holds no collective, so the same graph serves 1 and N ranks.
Per-layer generator noise (networks.py:281-286) is drawn inside the graph from torch's graph-safe Philox stream (fresh values every
replay).  Reference: train.py:56-110 is the region; the reference itself is eager PyTorch.
"""
import numpy as np
import torch


def freeze_host_objects():
    """Call once after the first training step(s): moves every Python object alive now — the networks' ~270 000 modules, launch plans, packed
    weight handles — into the collector's permanent generation (``gc.freeze``).  A full collection otherwise walks all of them (measured
    73 ms) whenever the young generations overflow, about once per 20 steps, on the thread that launches the step's ~650 kernels and is barely
    ahead of the GPU: one 160-250 ms step among 120 ms ones (the +4 % between a 5-step and a 20-step timing of round 3).  Afterwards a full
    pass only sees objects created since (0.01 ms).  The step itself leaves no reference cycles behind (tools/probes/gc_cycles.py).
    A program that later drops a whole graph and builds another calls ``gc.unfreeze()`` first (frozen objects are still freed by reference
    counting; only a cycle among them would wait for the unfreeze), as bench.py does between its workloads."""
    import gc
    gc.collect()
    gc.freeze()


def forward(g, z, alpha_for_graph, clamp=False, layers=None, content=False):
    """train.py:56-101 on DEVICE inputs: both generator passes, the regressor on the original, epsilon and the walk; no host
    synchronisation.  Returns (feed_dict for optimizeParametersAll, dict of device tensors).  ``content``: the step will take the content
    loss: the VGG taps of the original image start now, beside the regressor and the second generator pass (graph.prefetch_content_taps)."""
    w = g.get_w(z)
    x0 = g.get_logits({'w': w})
    if content:
        g.prefetch_content_taps(x0)
    a0 = g.get_reg_preds(x0, keep_feats=True)         # --attr_keep: the original's pooled features stay for the loss (graph.get_keep_feats)
    if clamp:
        target, eps = g.get_alphas_clamped(a0, alpha_for_graph)
    else:
        target, eps = alpha_for_graph, g.get_alphas(a0, alpha_for_graph)
    w1 = g.get_w_new_tensor(w, eps, layers=layers)
    x1 = g.get_logits({'w': w1})
    return {'w': w1, 'org': x0, 'logit': x1, 'alpha': target}, dict(x0=x0, x1=x1, a0=a0, eps=eps)


def forward_backward(g, z, alpha_for_graph, no_content_loss=False, no_gan_loss=False, clamp=False, layers=None):
    """``forward`` + the loss and backward of optimizeParametersAll (transform_base.py:459-488), without its all-reduce / Adam tail.
    Leaves d loss / d walk in ``walk.grad``."""
    feed, r = forward(g, z, alpha_for_graph, clamp=clamp, layers=layers, content=not no_content_loss)
    g.optimizers.zero_grad()
    loss = g.get_w_loss(feed, no_content_loss, no_gan_loss)
    loss.backward()
    r.update(loss=loss.detach(), terms=g.last_terms)
    return r


class _StagedInputs:
    """The static device inputs of a captured step — ``z`` [B, dim_z] and ``alpha`` [B, n_attr] — and their refill from the host."""

    def _init_inputs(self, dev, batch, dim_z, n_attr):
        self.z = torch.zeros(batch, dim_z, device=dev)
        self.alpha = torch.zeros(batch, n_attr, device=dev)
        # pinned staging ring: the host runs several replays ahead of the GPU (no per-step sync in bench.py / trainer --no_log_sync), so a
        # slot is rewritten only after the H2D copies that read it have run (one event per slot)
        self._ring = [(torch.zeros(batch, dim_z).pin_memory(), torch.zeros(batch, n_attr).pin_memory(), torch.cuda.Event()) for _ in range(4)]
        self._ring_used = [False] * len(self._ring)
        self._slot = 0

    def load(self, zs, alpha):
        """Host -> the graph's static inputs (pinned staging ring, asynchronous on the current stream)."""
        i = self._slot
        self._slot = (i + 1) % len(self._ring)
        stage_z, stage_a, ev = self._ring[i]
        if self._ring_used[i]:
            ev.synchronize()                                  # the copies that last read this slot have completed
        stage_z.copy_(torch.as_tensor(np.asarray(zs), dtype=torch.float32))
        stage_a.copy_(torch.as_tensor(np.asarray(alpha), dtype=torch.float32))
        self.z.copy_(stage_z, non_blocking=True)
        self.alpha.copy_(stage_a, non_blocking=True)
        ev.record()
        self._ring_used[i] = True


def record(device, step, warmup=2, before_capture=None):
    """Record one call of ``step()`` into a hipGraph (HIP stream capture through ``torch.cuda.graph``).  The protocol, once, for every recorded
    step of the package: ``max(warmup, 1)`` calls on a side stream (allocator pools, split-K workspaces, lazily packed weights: what capture
    cannot do), that stream joined both ways and the device synchronised, ``before_capture()`` (the callers' ``zero_grad(set_to_none=True)``:
    the gradients then become static tensors of the graph's pool), one call inside the capture.  Returns (graph, what the captured call returned,
    keep-alive list): the graph's kernel nodes hold RAW pointers into the split-K workspaces of conv._WS, allocated during warm-up outside the
    graph's pool, so the caller keeps that list for as long as the graph, even if a later eager launch replaces a dict entry with a larger one.

    Two rules for ``step``.  The warm-up runs loss and backward only, never an update: the walk (or W+), the optimiser state and the fp16 scaler
    are what an eager run starts from (a step that records its update makes it only under ``torch.cuda.is_current_stream_capturing()``).  And
    a recording meant to be ONE stream holds nothing attached to the autograd graph across the warm-up, so such a step returns detached tensors:
    a survivor keeps the leaves' gradient accumulators on the warm-up's stream, and the capture would fork to that stream to run them."""
    from . import conv
    s = torch.cuda.Stream(device=device)
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(max(warmup, 1)):
            step()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    if before_capture is not None:
        before_capture()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step()
    return graph, out, list(conv._WS.values())


class _CapturedWalkStep(_StagedInputs):
    """A walk graph's forward + backward (``self._step()``, on the static inputs) recorded once; every call loads the inputs, replays, points the
    walk's ``.grad`` at the graph's static gradient tensors and runs the graph's ``walk_update`` (all-reduce, optimiser step) outside the graph."""

    def _record(self, g, batch, n_attr, warmup):
        self.g = g
        self._init_inputs(g.device, batch, g.dim_z, n_attr)
        self.graph, self.out, self._ws_keep = record(g.device, self._step, warmup, lambda: g.optimizer.zero_grad(set_to_none=True))
        self.grads = [p.grad for p in g.walk.parameters()]          # static tensors inside the graph's pool, rewritten by every replay

    def __call__(self, zs=None, alpha=None, optimize=True):
        if zs is not None:
            self.load(zs, alpha)
        self.graph.replay()
        for p, gr in zip(self.g.walk.parameters(), self.grads):      # the optimiser reads p.grad
            p.grad = gr
        if optimize:
            self.g.walk_update()
        o = dict(self.out)
        o['grad'], o['grads'] = self.grads[0], self.grads
        return o


class CapturedStep(_CapturedWalkStep):
    """``step(zs, alpha)`` == selfcheck.run_step(g, zs, alpha, ...) with the forward+backward replayed from one hipGraph (the three loss branches
    fork from and join the captured stream)."""

    def __init__(self, g, batch, n_attr, no_content_loss=False, no_gan_loss=False, clamp=False, layers=None, warmup=2):
        self._flags = dict(no_content_loss=no_content_loss, no_gan_loss=no_gan_loss, clamp=clamp, layers=layers)
        self._record(g, batch, n_attr, warmup)

    def _step(self):
        return forward_backward(self.g, self.z, self.alpha, **self._flags)


class CapturedZStep(_CapturedWalkStep):
    """``step(zs, alpha_delta)`` == pggan.walk_training_step(g, zs, alpha_delta, ...) on the PGGAN graph (BASELINE config 1) with
    pggan.walk_forward_backward replayed from one hipGraph: the no-grad first pass, the clamp pair on the device, the walk in z, the second
    generator pass, zero_grad, loss and backward, all on one stream (no loss-branch forks: the recorded graph is a chain) and without noise.
    The GAN term cannot be evaluated on this graph (pggan.py) and is off."""

    def __init__(self, g, batch, n_attr, no_content_loss=False, warmup=2):
        self.no_content_loss = bool(no_content_loss)
        init_state = getattr(g.optimizer, 'init_state', None)
        if init_state is not None:
            init_state()                                                   # GuardedAdam: moments, counters and guard words outside the graph's pool
        self._record(g, batch, n_attr, warmup)

    def _step(self):
        """One pggan.walk_forward_backward on the static inputs -> its results, detached (``record``'s second rule)."""
        from . import pggan
        loss, x0, x1, a0, target = pggan.walk_forward_backward(self.g, self.z, self.alpha, no_content_loss=self.no_content_loss, no_gan_loss=True)
        return dict(loss=loss.detach(), x0=x0.detach(), x1=x1.detach(), a0=a0.detach(), target=target.detach(), terms=self.g.last_terms)


class CapturedRegressorStep(_StagedInputs):
    """One optimiser step of the attribute regressor (regressor_train.train_step_resident on a resident TrainableResNet50, or on the 16-bit
    TrainableResNet50H8 of a library with l2i_repack_planes_h8: its loss scaler then runs inside the graph as well) recorded into ONE
    stream of one hipGraph: (gather,) forward, loss, backward, guarded Adam, in-place repack.  The optimiser is inside the graph because its
    state is on the device (optim.GuardedAdam: counters included) and its table of pointers never changes (the model's gradient arena);
    ``record``'s rule holds: the warm-up runs forward, loss and backward only — no update, no repack, and the BatchNorm running statistics
    and batch counters stay as they are (model.track_stats) — and the update is recorded only while the stream is capturing.

    Inputs: ``dataset`` None — ``step(data, label)`` stages host tensors [B, 3, S, S] / [B, 40] through the pinned ring of ``_StagedInputs``;
    a regressor_train.DeviceDataset — ``step(idx=...)`` copies B checked int64 indices and the graph's first node gathers the batch
    (l2i_batch_from_u8_f32).  Returns the loss of the step, a device scalar that the next replay overwrites."""

    def __init__(self, model, optimizer, batch, size, dataset=None, warmup=2):
        from . import regressor_train as RT
        if not getattr(model, 'resident', False):
            raise ValueError('CapturedRegressorStep records a resident model (TrainableResNet50(..., resident=True))')
        if not hasattr(optimizer, 'init_state'):
            raise ValueError('CapturedRegressorStep records a device-side optimiser (regressor_train.make_optimizer(model, guarded=True))')
        if getattr(model, 'planes_kernel', True) is False or getattr(model, 'stem_kernel', True) is False:
            raise ValueError('CapturedRegressorStep: this library repacks the 16-bit planes with torch ops that allocate; it cannot be recorded')
        optimizer.init_state()                                             # moments, counters and guard words outside the graph's pool
        self.model, self.optimizer, self.dataset, self.batch = model, optimizer, dataset, batch
        n_out = model.fc_w.shape[0]
        self._init_inputs(model.device, batch, 3 * size * size, n_out)
        self.data, self.label = self.z.view(batch, 3, size, size), self.alpha
        self.idx = torch.zeros(batch, dtype=torch.long, device=model.device) if dataset is not None else None

        def step():
            capturing = torch.cuda.is_current_stream_capturing()
            if dataset is not None:
                dataset.gather(self.idx, self.data, self.label)
            model.track_stats = capturing
            try:
                return RT.train_step_resident(model, optimizer, self.data, self.label, update=capturing).detach()
            finally:
                model.track_stats = True
        self.graph, self.loss, self._ws_keep = record(model.device, step, warmup)

    def __call__(self, data=None, label=None, idx=None):
        if self.dataset is not None:
            idx = torch.as_tensor(idx, dtype=torch.long).reshape(-1)
            assert idx.numel() == self.batch
            self.idx.copy_(idx, non_blocking=True)
        else:
            self.load(torch.as_tensor(data, dtype=torch.float32).reshape(self.batch, -1).cpu(), torch.as_tensor(label, dtype=torch.float32).cpu())
        self.graph.replay()
        return self.loss
