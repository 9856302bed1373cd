"""The bits of q_sample, the dense guided step and the DDIM step with their noise read from a buffer (csrc/step.hip through
ipdm_q_sample / ipdm_ddpm_step / ipdm_ddim_step), pinned by a fixture: tests/golden/step_bits.npz holds inputs made on the host
and the outputs one build gave for them (tools/record_step_bits.py); every build since must give the same, torch.equal.  The
forms of these ops that draw their noise in registers are chained to these by the torch.equal tests of
test_gpu_native_reverse.py, test_gpu_native_sparse.py and test_gpu_adaptive_per_slice.py.

The 40x24 cases (n % 4 == 0: q_sample, the dense step, the DDIM step) also run with every tensor one float into padded
storage, so that no pointer is 16-byte aligned: the kernels' scalar path must give the bits of the 16-byte one."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import record_step_bits as rec                                  # noqa: E402

CASES = rec.cases()


@pytest.fixture(scope="module")
def golden():
    with np.load(os.path.join(ROOT, "tests", "golden", "step_bits.npz")) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def runner(golden):
    r = rec.Runner(golden)
    yield r
    r.close()


def _equal(a, b):
    return torch.equal(torch.from_numpy(a), torch.from_numpy(b))


def test_the_fixture_has_every_case_and_reproducible_inputs(golden):
    assert sorted(k[4:] for k in golden if k.startswith("out_")) == sorted(c[0] for c in CASES)
    for k, v in rec.make_inputs().items():
        assert _equal(golden[k], v), k


@pytest.mark.parametrize("key,op,shape,args", CASES, ids=[c[0] for c in CASES])
def test_step_bits_equal_the_recorded_ones(runner, golden, key, op, shape, args):
    assert _equal(runner.run(op, shape, args), golden["out_" + key]), key


@pytest.mark.parametrize("key,op,shape,args", [c for c in CASES if c[2] == (40, 24)], ids=[c[0] for c in CASES if c[2] == (40, 24)])
def test_unaligned_pointers_give_the_bits_of_aligned_ones(runner, golden, key, op, shape, args):
    got = runner.run(op, shape, args, shift=1)
    assert _equal(got, runner.run(op, shape, args)), key
    assert _equal(got, golden["out_" + key]), key
