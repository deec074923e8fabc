"""The speculative Jacobian evaluation of the BA solver against its "off" form.

By default (openmvg_amd/csrc/mvgx_ba.hip, `speculate`) the Jacobian at x + delta is launched before the host has decided on the step,
gated on the device by the accept word; MVGX_BA_SPECULATE=0 launches it after the host's decision, the order before round 6. The
arithmetic at every x is the same, so the two forms must agree BIT FOR BIT after every step - cost, successful steps, termination and
parameters - and a whole solve must follow the restatement's schedule (iterations, termination, RMSE within RMSE_TOL).

The test hook mvgx_debug_ba_speculation (BaContext.speculation) counts {evaluations launched ahead, consumed as the next Jacobian, gate
stayed shut}: every case asserts that the path it claims ran - the look-ahead with the default form, nothing with MVGX_BA_SPECULATE=0 and
under the exclusion rules (pose priors, several shards, MVGX_BA_SEPARATE_COST=1, MVGX_BA_POLL_SCALARS=0). The emulation maps host memory for the device
(hipHostGetDevicePointer), so the polled scalars and with them the look-ahead run there too; the gpu-marked twins run the same cases.

Each option set switches off the termination tests it does not exercise (tolerance 0), so that the termination code names the test
that fired: termination 0 with only function_tolerance > 0 is the function-tolerance test, and so on."""
import numpy as np
import pytest

from openmvg_amd import ba, synth
from tests import _emu, _oracle
from tests.test_ba_emu_cpu import RMSE_TOL
from tests.test_ba_update import _perturbed

SCENES = {
    "clean": dict(n_cams=20, n_points=800, track_len=7, model=1, seed=41),                              # test_trajectory_equals_oracle's
    "huber_outliers": dict(n_cams=9, n_points=300, track_len=9, model=2, seed=43, outlier_frac=0.08),   # test_trajectory_equals_oracle's
}
_OFF = dict(function_tolerance=0.0, parameter_tolerance=0.0, gradient_tolerance=0.0, min_radius=0.0)
OPTIONS = {   # name -> (options, expected termination)
    "function_tolerance": (dict(_OFF, function_tolerance=1e-4, max_num_iterations=50), 0),
    "parameter_tolerance": (dict(_OFF, parameter_tolerance=1e-2, max_num_iterations=50), 0),
    "max_num_iterations": (dict(_OFF, max_num_iterations=3), 1),
    # a trust region so wide that the LM diagonal cannot make the gauge-free reduced system definite: the linear solve fails, the step
    # is invalid, and one such step ends the solve (the C ABI then returns MVGX_ERR_NUMERIC with the summary filled)
    "max_consecutive_invalid_steps": (dict(_OFF, function_tolerance=1e-4, max_num_iterations=50, initial_radius=1e30, max_radius=1e32,
                                           max_consecutive_invalid_steps=1), 2),
}


def _scene(name, priors=False):
    sc = synth.ba_scene(**SCENES[name])
    return synth.add_pose_priors(sc, sigma=0.005, huber_a=2e-4, every=2) if priors else sc


def _params_bytes(p):
    return tuple(a.tobytes() for a in p)


def _solved(sc, opts, devices=None):
    """(summary, parameters, speculation counts); MVGX_ERR_NUMERIC - the invalid-step ending - is a result here, not an error"""
    import ctypes as C
    from openmvg_amd import _capi
    ctx = ba.BaContext(sc) if devices is None else ba.BaContext(sc, devices=devices)
    try:
        s = _capi.BaSummary()
        rc = _capi.lib().mvgx_ba_solve(ctx._h, C.byref(ba.default_options(**opts)), C.byref(s))
        assert rc in (_capi.MVGX_OK, _capi.MVGX_ERR_NUMERIC), rc
        assert (rc == _capi.MVGX_ERR_NUMERIC) == (s.termination == 2), (rc, s.termination)
        return s, _params_bytes(ctx.read_params()), ctx.speculation()
    finally:
        ctx.close()


def _both_forms(monkeypatch, fn):
    """(off form, default form) of fn()"""
    with monkeypatch.context() as m:
        m.setenv("MVGX_BA_SPECULATE", "0")
        off = fn()
    monkeypatch.delenv("MVGX_BA_SPECULATE", raising=False)
    return off, fn()


def _same_solve(s_off, s_on):
    for f in ("num_iterations", "num_successful_steps", "termination", "initial_cost", "final_cost", "final_rmse"):
        assert getattr(s_off, f) == getattr(s_on, f), (f, getattr(s_off, f), getattr(s_on, f))


def check_termination(monkeypatch, scene, opt, opts=None):
    """a solve that ends by the named test: both forms bit-identical, the restatement's schedule, and the look-ahead's counts"""
    sc = _scene(scene)
    opts, termination = (OPTIONS[opt][0] if opts is None else opts), OPTIONS[opt][1]
    (s_off, p_off, n_off), (s_on, p_on, n_on) = _both_forms(monkeypatch, lambda: _solved(sc, opts))
    _same_solve(s_off, s_on)
    assert p_off == p_on
    assert n_off == (0, 0, 0), n_off
    rc, osum, *_ = _oracle.port_ba_solve(sc, options=_oracle.default_ba_options(**opts))
    assert (rc == 0) == (termination != 2), rc
    assert (s_on.num_iterations, s_on.num_successful_steps, s_on.termination) == (osum.num_iterations, osum.num_successful_steps, osum.termination)
    assert abs(s_on.final_rmse - osum.final_rmse) < RMSE_TOL
    assert s_on.termination == termination, (opt, s_on.termination, s_on.num_iterations)
    launched, consumed, shut = n_on
    assert consumed + shut <= launched, n_on
    if opt == "max_consecutive_invalid_steps":
        # the invalid step was launched ahead like every other; the device saw it fail and kept the gate shut
        assert consumed == 0 and launched == shut == s_on.num_iterations >= 1, n_on
        return s_on, n_on
    assert consumed > 0, n_on
    if opt == "max_num_iterations":
        # every iteration but the last launches (its evaluation would never be used): the last accepted step launches nothing
        assert s_on.num_iterations == opts["max_num_iterations"] and launched == opts["max_num_iterations"] - 1, n_on
    else:
        assert s_on.num_iterations < opts["max_num_iterations"]
        # the last step was launched ahead and the device kept its gate shut: a tolerance test ended the solve there, or the step was invalid
        assert launched == s_on.num_iterations and shut >= 1, n_on
    return s_on, n_on


def check_rejected_steps(monkeypatch):
    """the Huber-outlier scene from a wide first trust region rejects steps: each rejected step's look-ahead stays behind its shut gate"""
    opts = dict(OPTIONS["function_tolerance"][0], initial_radius=1e8, max_radius=1e16)
    s_on, (launched, consumed, shut) = check_termination(monkeypatch, "huber_outliers", "function_tolerance", opts)
    # iterations = accepted steps (num_successful_steps less iteration zero) + rejected steps + the step the function test ended on
    rejected = s_on.num_iterations - (s_on.num_successful_steps - 1) - 1
    assert rejected >= 1 and consumed == s_on.num_successful_steps - 1 and shut == rejected + 1, (s_on.num_iterations, s_on.num_successful_steps, launched, consumed, shut)


def _stepped(sc, opts, n_steps, perturb_after=None):
    """after each lm_iteration(): (cost, successful steps, termination, parameters); with perturb_after = k the scene is replaced by a
    perturbed one of the same structure after step k (evaluate(), residuals(), update() in between)"""
    ctx = ba.BaContext(sc)
    out = []
    try:
        for k in range(n_steps):
            s = ctx.lm_iteration(ba.default_options(**opts))
            out.append((s.final_cost, s.num_successful_steps, s.termination, _params_bytes(ctx.read_params())))
            if perturb_after == k:
                out.append(ctx.evaluate())
                out.append(ctx.residuals().tobytes())
                assert ctx.update(_perturbed(sc, 5))
                out.append(ctx.evaluate())
        return out, ctx.speculation()
    finally:
        ctx.close()


def check_stepping(monkeypatch, scene, perturb_after=None, n_steps=6):
    sc = _scene(scene)
    opts = dict(_OFF, max_num_iterations=50)
    (off, n_off), (on, n_on) = _both_forms(monkeypatch, lambda: _stepped(sc, opts, n_steps, perturb_after))
    assert len(off) == len(on)
    for k, (a, b) in enumerate(zip(off, on)):
        assert a == b, k
    assert n_off == (0, 0, 0) and n_on[0] > 0 and n_on[1] > 0, (n_off, n_on)


def check_excluded(monkeypatch, rule):
    """the exclusion rules of the look-ahead take the off path: count 0, same results as MVGX_BA_SPECULATE=0; the scalars of a step
    brought by copy + synchronise ("copied_scalars") change their transport and no operation: the same results as with the polled ones"""
    opts = OPTIONS["function_tolerance"][0]
    sc = _scene("clean", priors=rule == "pose_priors")
    devices = [0, 0] if rule == "two_shards" else None
    if rule == "separate_cost":
        monkeypatch.setenv("MVGX_BA_SEPARATE_COST", "1")
    if rule == "copied_scalars":
        s_polled, p_polled, _ = _solved(sc, opts)
        monkeypatch.setenv("MVGX_BA_POLL_SCALARS", "0")
    (s_off, p_off, n_off), (s_on, p_on, n_on) = _both_forms(monkeypatch, lambda: _solved(sc, opts, devices))
    _same_solve(s_off, s_on)
    assert p_off == p_on
    assert n_off == n_on == (0, 0, 0), (n_off, n_on)
    assert s_on.num_iterations > 1
    if rule == "copied_scalars":
        _same_solve(s_polled, s_on)
        assert p_polled == p_on


# ---- emulated ----
@pytest.mark.parametrize("opt", sorted(OPTIONS))
def test_termination_off_and_default_forms_are_bit_identical_emulated(opt, monkeypatch):
    with _emu.emulated():
        check_termination(monkeypatch, "clean", opt)


def test_rejected_steps_emulated(monkeypatch):
    with _emu.emulated():
        check_rejected_steps(monkeypatch)


@pytest.mark.parametrize("scene", sorted(SCENES))
def test_stepping_off_and_default_forms_are_bit_identical_emulated(scene, monkeypatch):
    with _emu.emulated():
        check_stepping(monkeypatch, scene, n_steps=4)


def test_stepping_around_evaluate_residuals_update_emulated(monkeypatch):
    with _emu.emulated():
        check_stepping(monkeypatch, "clean", perturb_after=1, n_steps=4)


@pytest.mark.parametrize("rule", ["pose_priors", "separate_cost", "copied_scalars"])
def test_excluded_contexts_take_the_off_path_emulated(rule, monkeypatch):
    with _emu.emulated():
        check_excluded(monkeypatch, rule)


# ---- MI355X ----
@pytest.mark.gpu
@pytest.mark.parametrize("scene", sorted(SCENES))
@pytest.mark.parametrize("opt", sorted(OPTIONS))
def test_termination_off_and_default_forms_are_bit_identical(scene, opt, monkeypatch):
    if scene == "huber_outliers" and opt == "max_consecutive_invalid_steps":
        pytest.skip("the invalid-step ending is exercised on the clean scene")
    check_termination(monkeypatch, scene, opt)


@pytest.mark.gpu
def test_rejected_steps(monkeypatch):
    check_rejected_steps(monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("scene", sorted(SCENES))
def test_stepping_off_and_default_forms_are_bit_identical(scene, monkeypatch):
    check_stepping(monkeypatch, scene)


@pytest.mark.gpu
def test_stepping_around_evaluate_residuals_update(monkeypatch):
    check_stepping(monkeypatch, "clean", perturb_after=2)


@pytest.mark.gpu
@pytest.mark.parametrize("rule", ["pose_priors", "separate_cost", "two_shards", "copied_scalars"])
def test_excluded_contexts_take_the_off_path(rule, monkeypatch):
    check_excluded(monkeypatch, rule)
