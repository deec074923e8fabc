"""CPU: mvgx_relative_pose_from_essential - the device code of openmvg_amd/csrc/mvgx_relative_pose.h under the HIP emulation
(tests/_emu.py) - on the hard matrices of tests/_relative_pose_hard_cases.py against the 50-digit decomposition of
tests/_relative_pose_truth.py: every family under all four methods. The -m gpu twin of this file is
tests/test_relative_pose_hard_gpu.py."""
import pytest

from tests import _emu
from tests import _relative_pose_hard_cases as hard


@pytest.fixture(autouse=True)
def _emulated():
    with _emu.emulated():
        yield


@pytest.mark.parametrize("family", hard.FAMILIES)
@pytest.mark.parametrize("method", range(4))
def test_hard_family(method, family):
    hard.check_family(family, method)


@pytest.mark.parametrize("method", range(4))
def test_zero_and_non_finite_matrices_give_no_pose(method):
    hard.check_no_motion(method)
