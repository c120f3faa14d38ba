"""The host logic of the inference flags (latent2im_amd/vis.py) — no GPU."""
import argparse

import pytest

from latent2im_amd import conv, vis


def test_precision_flag_resolves_against_the_training_runs_record():
    for recorded, want in ((None, 'f32'), ('f16', 'f16'), ('bf16', 'bf16')):
        conf = argparse.Namespace(precision=recorded)
        assert vis.resolve_precision('train', conf) == want
        assert vis.resolve_precision('bf16', conf) == 'bf16' and vis.resolve_precision('f32', conf) == 'f32'
        assert vis.resolve_precision(None, conf) == conv.PRECISION          # no flag: the process keeps what it has
    assert vis.resolve_precision('train', argparse.Namespace()) == 'f32'     # an opt.yml from before the training flag existed


def test_precision_flag_choices():
    p = argparse.ArgumentParser()
    vis.add_precision_flag(p)
    assert p.parse_args([]).precision is None
    assert [p.parse_args(['--precision', v]).precision for v in vis.PRECISIONS] == ['f32', 'f16', 'bf16', 'train']
    with pytest.raises(SystemExit):
        p.parse_args(['--precision', 'fp8'])
