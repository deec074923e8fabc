"""GPU: mvgx_relative_pose_from_essential and mvgx_relative_pose_robust on the MI355X against the compiled reference's outputs
(tests/golden/relative_pose_golden.npz), the float64 restatement (tests/_relative_pose_ref.py) and, for the angular pose stage, the
compiled functor of oracle/_ref. The cases are in tests/_relative_pose_cases.py; the CPU twin (emulation) is
tests/test_relative_pose_emu_cpu.py."""
import pytest

from tests import _relative_pose_cases as cases

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("explicit_lists", [True, False])
@pytest.mark.parametrize("method", range(4))
def test_lane_and_row_edges(method, explicit_lists):
    cases.check_edges(method, explicit_lists)


@pytest.mark.parametrize("method", range(4))
def test_ratio_edge(method):
    cases.check_ratio(method)


@pytest.mark.parametrize("method", range(4))
def test_no_solution(method):
    cases.check_no_solution(method)


def test_arguments():
    cases.check_arguments()


@pytest.mark.parametrize("setting", [0, 1])
def test_robust_pinhole(setting):
    cases.check_robust_pinhole(setting)


def test_robust_angular():
    cases.check_robust_angular()


def test_angular_pose_stage_against_compiled_functor():
    cases.check_angular_pose_stage_against_oracle()


def test_twenty_inliers_pass_here_and_fail_in_the_filter():
    cases.check_twenty_inliers()


def test_tiny_scene():
    cases.check_tiny_scene()
