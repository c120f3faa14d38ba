"""The optimiser tail of the walk step on the fp16 path: a dynamic loss scale and an Adam that skips non-finite steps, both on the device.

The reference ends every step with ``self.optimizers.step()`` (transform_base.py:487-488; torch.optim.Adam(lr, betas=(0.5, 0.99)), :329-331) on the
walk.  Run under autocast — what BASELINE configs[4] ("fp16 MFMA") amounts to for the reference — that call would go through a torch GradScaler:
scale the loss, look for inf / NaN in the gradients, skip the update and halve the scale if there is one, double it after ``growth_interval`` clean
steps.  torch's GradScaler reads its ``found_inf`` back to the host before every optimiser step; the step here never synchronises (train.py:110 is
the only sync of the reference loop, and the hipGraph replay of config 5 has none), so the same semantics are kept in three device words
(csrc/l2i_optim.hip).

``LossScaler``  — per graph: the STATIC per-branch exponents of nets16.loss_scale_for (each loss branch's largest gradient map near 2^5) times ONE
                  dynamic power of two ``scale[0]`` (1.0 at start).  Every branch multiplies the gradient it receives by static * dynamic
                  (a device tensor, so a captured hipGraph sees every update) and the generator's latent gradient by the inverse: walk.grad is the
                  true gradient, or non-finite if anything overflowed on the way.
``GuardedAdam`` — torch.optim.Adam whose step() is one launch of l2i_adam_guarded_f32 for a single parameter tensor (finite check, update or
                  skip, scale-state update) and, for several tensors, two library calls per 16 of them: l2i_nonfinite_flag_multi_f32 over every
                  gradient, then l2i_adam_guarded_multi_f32 (a multi-block update and a one-wave tail).  Same state layout as torch's
                  (exp_avg, exp_avg_sq, step) so state_dict() round-trips.
``GuardedSGD``  — torch.optim.SGD(lr, momentum) the same way on l2i_sgd_guarded_f32 (BP.py:140, the inversion's 'GD'): torch's momentum_buffer plus a
                  device-side ``step`` that tells the kernel whether the buffer is still to be initialised, so a captured graph replays the step.
"""
import torch

from . import _lib


class LossScaler:
    GROWTH, BACKOFF = 2.0, 0.5

    def __init__(self, log2, device, growth_interval=2000, max_log2=8):
        """``log2``: dict(R, V, D, G) of static exponents.  ``growth_interval``: clean steps before the dynamic factor doubles (torch's default);
        ``max_log2``: it never grows beyond 2^max_log2 (the static exponents already sit eleven octaves under fp16's largest number)."""
        self.log2 = dict(log2)
        self.device = device
        self.growth_interval = int(growth_interval)
        self.max_scale = float(2.0 ** max_log2)
        self.scale = torch.tensor([1.0, 1.0], dtype=torch.float32, device=device)          # [dynamic factor, its inverse]
        self.state = torch.zeros(4, dtype=torch.int32, device=device)                      # L2I_LS_FOUND / TRACKER / SKIPPED / STEPS
        self.dyn, self.inv_dyn = self.scale[0:1], self.scale[1:2]                          # views: what the captured graph multiplies by

    def static(self, key):
        return float(2.0 ** self.log2[key])

    def stats(self):
        """dict(scale, tracker, skipped, steps) — a host read (synchronises): logging and tests only."""
        st = self.state.tolist()
        return dict(scale=float(self.scale[0]), tracker=st[1], skipped=st[2], steps=st[3])


def _guard_flags(self, device):
    """(state words, scale pair or None) of a guarded optimiser: the scaler's, or four words of its own."""
    if self.scaler is not None:
        return self.scaler.state, self.scaler.scale
    if self._own_state is None or self._own_state.device != device:
        self._own_state = torch.zeros(4, dtype=torch.int32, device=device)
    return self._own_state, None


def _init_state(self):
    """Allocate every parameter's state and the guard's own words now and not in the first step(): before a graph capture, whose pool they
    must not come from."""
    for group in self.param_groups:
        for p in group['params']:
            _check_param(p, type(self).__name__)
            self._state_of(p)
            self._flags(p.device)


def _check_param(p, who):
    if p.dtype != torch.float32 or not p.is_cuda or not p.is_contiguous() or (p.grad is not None and p.grad.dtype != torch.float32):
        raise _lib.L2IError('%s updates contiguous float32 GPU parameters only' % who)


def _guarded_step(opt, todo, launch):
    """The launches of one guarded step over ``todo`` = [(p, group, state)]: multi-tensor steps flag every gradient first, the last launch advances
    the scale state.  ``launch(p, g, group, st, guard, stream)`` enqueues one update; ``guard`` is the entry point's tail from check_self to last."""
    if not todo:
        return None
    state, scale = opt._flags(todo[0][0].device)
    sc = opt.scaler
    single = len(todo) == 1
    stream = _lib.stream_ptr()
    if not single:
        for p, _, _ in todo:
            g = p.grad if p.grad.is_contiguous() else p.grad.contiguous()
            _lib.call('l2i_nonfinite_flag_f32', _lib.fptr(g), g.numel(), _lib.ptr(state), stream=stream)
    for i, (p, group, st) in enumerate(todo):
        g = p.grad if p.grad.is_contiguous() else p.grad.contiguous()
        launch(p, g, group, st, (1 if single else 0, _lib.ptr(state), _lib.ptr(scale), float(sc.GROWTH if sc else 2.0), float(sc.BACKOFF if sc else 0.5),
                                 int(sc.growth_interval if sc else 0), float(sc.max_scale if sc else 1.0), 1 if i == len(todo) - 1 else 0), stream)
    return None


class GuardedAdam(torch.optim.Adam):
    """torch.optim.Adam(params, lr, betas) for float32 CUDA parameters with the update on l2i_adam_guarded_f32 (one tensor) or
    l2i_adam_guarded_multi_f32 (several): skipped as a whole when any gradient of the step is non-finite; ``scaler`` (a LossScaler or None) is
    advanced by the last launch of the step."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, scaler=None):
        super().__init__(params, lr=lr, betas=betas, eps=eps)
        self.scaler = scaler
        self._own_state = None

    _flags = _guard_flags

    def _state_of(self, p):
        st = self.state[p]
        if len(st) == 0:
            st['step'] = torch.zeros((), dtype=torch.float32, device=p.device)
            st['exp_avg'] = torch.zeros_like(p, memory_format=torch.preserve_format)
            st['exp_avg_sq'] = torch.zeros_like(p, memory_format=torch.preserve_format)
        elif not st['step'].is_cuda:                           # a state_dict saved by torch's own Adam keeps the counter on the host
            st['step'] = st['step'].to(device=p.device, dtype=torch.float32)
        return st

    init_state = _init_state

    @torch.no_grad()
    def step(self, closure=None):
        if closure is not None:
            raise NotImplementedError('GuardedAdam.step takes no closure (the reference calls optimizers.step() bare, transform_base.py:488)')
        todo = []
        for group in self.param_groups:
            if group.get('weight_decay', 0) or group.get('amsgrad', False) or group.get('maximize', False):
                raise NotImplementedError('GuardedAdam: plain Adam only (the reference uses lr and betas, transform_base.py:329-331)')
            for p in group['params']:
                if p.grad is None:
                    continue
                _check_param(p, 'GuardedAdam')
                todo.append((p, group, self._state_of(p)))

        if len(todo) > 1:
            return self._step_multi(todo)

        def launch(p, g, group, st, guard, stream):
            b1, b2 = group['betas']
            _lib.call('l2i_adam_guarded_f32', _lib.fptr(p), _lib.fptr(g), _lib.fptr(st['exp_avg']), _lib.fptr(st['exp_avg_sq']), _lib.fptr(st['step']),
                      p.numel(), float(group['lr']), float(b1), float(b2), float(group['eps']), *guard, stream=stream)
        return _guarded_step(self, todo, launch)

    def _step_multi(self, todo):
        """A step over several tensors: chunks of one param group and at most _lib.ADAM_MAX_TENSORS tensors; every chunk's gradients are flagged
        before the first update, the last update call advances the scale state."""
        state, scale = self._flags(todo[0][0].device)
        sc = self.scaler
        stream = _lib.stream_ptr()
        chunks, keep = [], []
        for p, group, st in todo:
            g = p.grad if p.grad.is_contiguous() else p.grad.contiguous()
            if not (st['exp_avg'].is_contiguous() and st['exp_avg_sq'].is_contiguous()):
                raise _lib.L2IError('GuardedAdam updates contiguous moments only')
            keep.append(g)
            row = _lib.AdamTensor(_lib.fptr(p), _lib.fptr(g), _lib.fptr(st['exp_avg']), _lib.fptr(st['exp_avg_sq']), _lib.fptr(st['step']), p.numel())
            if not chunks or chunks[-1][0] is not group or len(chunks[-1][1]) == _lib.ADAM_MAX_TENSORS:
                chunks.append((group, []))
            chunks[-1][1].append(row)
        tables = [(group, (_lib.AdamTensor * len(rows))(*rows), len(rows)) for group, rows in chunks]
        for _, table, count in tables:
            _lib.call('l2i_nonfinite_flag_multi_f32', table, count, _lib.ptr(state), stream=stream)
        for i, (group, table, count) in enumerate(tables):
            b1, b2 = group['betas']
            _lib.call('l2i_adam_guarded_multi_f32', table, count, float(group['lr']), float(b1), float(b2), float(group['eps']), _lib.ptr(state),
                      _lib.ptr(scale), float(sc.GROWTH if sc else 2.0), float(sc.BACKOFF if sc else 0.5), int(sc.growth_interval if sc else 0),
                      float(sc.max_scale if sc else 1.0), 1 if i == len(tables) - 1 else 0, stream=stream)
        return None


class GuardedSGD(torch.optim.SGD):
    """torch.optim.SGD(params, lr, momentum) — dampening 0, no Nesterov, no weight decay: BP.py:140 — for float32 CUDA parameters with the update on
    l2i_sgd_guarded_f32, guarded and scaled as GuardedAdam's.  State per parameter: torch's ``momentum_buffer`` and ``step``, a 0-dim float32 device
    tensor (0: the next applied step sets the buffer to the gradient, as torch's first step does)."""

    def __init__(self, params, lr=1e-3, momentum=0.0, scaler=None):
        super().__init__(params, lr=lr, momentum=momentum)
        self.scaler = scaler
        self._own_state = None

    _flags = _guard_flags

    def _state_of(self, p):
        st = self.state[p]
        buf = st.get('momentum_buffer')
        if buf is None:
            st['momentum_buffer'] = torch.zeros_like(p, memory_format=torch.contiguous_format)
            st['step'] = torch.zeros((), dtype=torch.float32, device=p.device)
        elif 'step' not in st:                                     # a state_dict saved by torch's own SGD: its buffer is already initialised
            st['step'] = torch.ones((), dtype=torch.float32, device=p.device)
        elif not st['step'].is_cuda:
            st['step'] = st['step'].to(device=p.device, dtype=torch.float32)
        if not st['momentum_buffer'].is_contiguous():
            st['momentum_buffer'] = st['momentum_buffer'].contiguous()
        return st

    init_state = _init_state

    @torch.no_grad()
    def step(self, closure=None):
        if closure is not None:
            raise NotImplementedError('GuardedSGD.step takes no closure (the reference calls optimizer.step() bare, BP.py:155)')
        todo = []
        for group in self.param_groups:
            if group.get('nesterov', False) or group.get('dampening', 0) or group.get('weight_decay', 0) or group.get('maximize', False):
                raise NotImplementedError('GuardedSGD: lr and momentum only (BP.py:140): no Nesterov, dampening, weight decay or maximize')
            for p in group['params']:
                if p.grad is None:
                    continue
                _check_param(p, 'GuardedSGD')
                todo.append((p, group, self._state_of(p)))

        def launch(p, g, group, st, guard, stream):
            _lib.call('l2i_sgd_guarded_f32', _lib.fptr(p), _lib.fptr(g), _lib.fptr(st['momentum_buffer']), _lib.fptr(st['step']), p.numel(),
                      float(group['lr']), float(group['momentum']), *guard, stream=stream)
        return _guarded_step(self, todo, launch)
