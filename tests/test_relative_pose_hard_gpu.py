"""GPU: mvgx_relative_pose_from_essential on the MI355X on the hard matrices of tests/_relative_pose_hard_cases.py - zero columns, equal
singular values, half turns, estimated matrices, scaled ones, offset and repeating lists - against the 50-digit decomposition of
tests/_relative_pose_truth.py, all four methods, every family one batch. The CPU twin (emulation) is
tests/test_relative_pose_hard_emu_cpu.py."""
import pytest

from tests import _relative_pose_hard_cases as hard

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("family", hard.FAMILIES)
@pytest.mark.parametrize("method", range(4))
def test_hard_family(method, family):
    hard.check_family(family, method)


@pytest.mark.parametrize("method", range(4))
def test_zero_and_non_finite_matrices_give_no_pose(method):
    hard.check_no_motion(method)
