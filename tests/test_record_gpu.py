"""capture.record alone: the protocol every recorded step of the package goes through, on a step of one kernel."""
import pytest
import torch

from latent2im_amd import capture, conv

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def _recorded(warmup):
    x = torch.arange(64, dtype=torch.float32, device=DEV)
    y = torch.zeros(64, dtype=torch.float32, device=DEV)
    events = []

    def step():
        events.append('step')
        y.copy_(x * 2 + 1)
        return y

    graph, out, keep = capture.record(torch.device(DEV, torch.cuda.current_device()), step, warmup, lambda: events.append('hook'))
    return x, y, events, graph, out, keep


def test_record_warms_up_runs_the_hook_once_and_captures_one_call():
    x, y, events, graph, out, keep = _recorded(2)
    assert events == ['step', 'step', 'hook', 'step']
    assert out is y
    ws = list(conv._WS.values())                                            # the workspaces alive at that moment, the very tensors
    assert len(keep) == len(ws) and all(a is b for a, b in zip(keep, ws))
    for fill in (3.0, -0.625):
        x.fill_(fill)
        y.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(y, torch.full((64,), fill * 2 + 1, device=DEV))
    assert events == ['step', 'step', 'hook', 'step']                        # a replay calls nothing on the host


def test_record_with_no_warmup_still_warms_up_once():
    x, y, events, graph, out, keep = _recorded(0)
    assert events == ['step', 'hook', 'step']
    x.copy_(torch.linspace(-1, 1, 64, device=DEV))
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(y, x * 2 + 1)
