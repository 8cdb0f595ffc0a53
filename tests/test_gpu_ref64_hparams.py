"""The HIP step-batch at the edges of its hyper-parameters against the float64 model: the cases of tests/test_ref64_hparams.py
(gamma 0 / 1, alpha 0 / 1, zero, negative and huge success rewards, step limits of 1 and 2, re-offer periods 0 .. 2^20 round
multiples of 2^19 and 2^20, count floors up to 2^30, weights of trained size, and the padded env order at 1000 envs), each plain
and with SPEC §12's interruption, on the 256- and the 64-env build."""
import pytest

from gpu_util import block_envs                               # noqa: F401  (the fixture)
from test_gpu_ref64 import GpuRunner
from test_gpu_ref64_interrupt import IntGpuRunner
from test_ref64_hparams import CASE_IDS, HP_CASES, hparam_case

pytestmark = pytest.mark.gpu

RUNNERS = {"plain": GpuRunner, "interrupting": IntGpuRunner}


@pytest.mark.parametrize("mode", list(RUNNERS))
@pytest.mark.parametrize("case", HP_CASES, ids=CASE_IDS)
@pytest.mark.parametrize("block_envs", [256, 64], indirect=True)
def test_hip_step_at_hyperparameter_edges(case, mode, block_envs):
    layouts = hparam_case(RUNNERS[mode], case, block_envs)
    if case["n"] == 1000:
        assert "padded" in layouts
