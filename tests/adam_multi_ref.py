"""A numpy model of one guarded multi-tensor Adam step (include/l2i.h: l2i_nonfinite_flag_multi_f32 + l2i_adam_guarded_multi_f32), the yardstick of
tests/test_adam_multi_cpu.py and tests/test_adam_multi_gpu.py.

State as the library keeps it: per tensor ``p, g, m, v`` (float32 arrays) and ``step`` (a float32 counter of its own: a loaded state_dict may
give every tensor another); per optimiser ``state`` = int32 [FOUND, TRACKER, SKIPPED, STEPS] and ``scale`` = float32 [factor, 1 / factor] or None.
The update is torch's _single_tensor_adam in float32 with the bias corrections in double; products and sums are rounded one by one here (numpy has
no fused multiply-add), which is within an ulp or two of the kernels' three fused ones: the GPU tests compare the kernels bit for bit with the
single-tensor kernel and hold them to 1e-6 against torch.optim.Adam, and use this model for what moves when."""
import numpy as np

FOUND, TRACKER, SKIPPED, STEPS = 0, 1, 2, 3
F = np.float32


def new_state():
    return np.zeros(4, np.int32), np.array([1.0, 1.0], np.float32)


def flag(tensors, state):
    """l2i_nonfinite_flag_multi_f32: FOUND = 1 if any gradient holds an inf / NaN; never cleared here."""
    if any(not np.isfinite(t['g']).all() for t in tensors):
        state[FOUND] = 1


def update(tensors, lr, beta1, beta2, eps, state, scale, growth=2.0, backoff=0.5, interval=0, max_scale=1.0, last=True):
    """l2i_adam_guarded_multi_f32: the update of every tensor unless FOUND is set, each with its own step counter; then the counters, and with
    ``last`` the scale state (torch._amp_update_scale_ under ``max_scale``) and the flag."""
    found = int(state[FOUND])
    if not found:
        for t in tensors:
            step = F(t['step'] + F(1))
            bc1 = 1.0 - float(F(beta1)) ** float(step)
            bc2 = 1.0 - float(F(beta2)) ** float(step)
            size, bc2s = F(float(F(lr)) / bc1), F(np.sqrt(bc2))
            g = t['g']
            t['v'][...] = F(beta2) * t['v'] + (F(1) - F(beta2)) * g * g
            t['m'][...] = t['m'] + (F(1) - F(beta1)) * (g - t['m'])
            denom = np.sqrt(t['v']) / bc2s + F(eps)
            t['p'][...] = t['p'] - size * (t['m'] / denom)
            t['step'] = step
    if last:
        if found:
            state[TRACKER] = 0
            state[SKIPPED] += 1
            if scale is not None:
                scale[0] *= F(backoff)
        else:
            tr = int(state[TRACKER]) + 1
            if interval > 0 and tr >= interval:
                state[TRACKER] = 0
                if scale is not None and F(scale[0] * F(growth)) <= F(max_scale):
                    scale[0] *= F(growth)
            else:
                state[TRACKER] = tr
        if scale is not None:
            scale[1] = F(1) / scale[0]
        state[STEPS] += 1
        state[FOUND] = 0


def step(tensors, lr, beta1, beta2, eps, state, scale, chunk=16, **kw):
    """GuardedAdam.step over one param group: every chunk flagged first, then updated; the last update advances the scale state."""
    chunks = [tensors[i:i + chunk] for i in range(0, len(tensors), chunk)]
    for c in chunks:
        flag(c, state)
    for i, c in enumerate(chunks):
        update(c, lr, beta1, beta2, eps, state, scale, last=i == len(chunks) - 1, **kw)
