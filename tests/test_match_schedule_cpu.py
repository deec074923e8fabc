"""CPU: the batch schedule of a matching run and the record order inside an XCD's slice, alone (openmvg_amd/csrc/mvgx_match_batch.h,
plain C++ without HIP).

tests/native/match_schedule_main.cpp is a stand-alone program (its own main, AddressSanitizer and UndefinedBehaviorSanitizer linked in: no
preloaded runtime). It checks the schedule over the sizes around the ramp's threshold, and the order over the record lists of
tests/_match_block_cases.py and random ones, into buffers of exactly the records' size, and asserts what its header lists. Pass = exit
status 0, its last line, and no sanitizer report."""
import os
import subprocess

from tests import _emu, _match_block_cases as cases

_NATIVE = os.path.join(_emu._HERE, "native")
_MAIN = os.path.join(_NATIVE, "match_schedule_main.cpp")
_HEADER = os.path.join(_emu._ROOT, "openmvg_amd", "csrc", "mvgx_match_batch.h")


def _build():
    out = os.path.join(_NATIVE, "_build", "match_schedule")
    if os.path.exists(out) and all(os.path.getmtime(d) <= os.path.getmtime(out) for d in (_MAIN, _HEADER)):
        return out
    os.makedirs(os.path.dirname(out), exist_ok=True)
    cxx = _emu._CLANG if os.path.exists(_emu._CLANG) else "clang++"
    subprocess.run([cxx, "-x", "c++", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                    "-g", "-O1", "-Wall", "-Werror", "-I" + os.path.dirname(_HEADER), _MAIN, "-o", out], check=True)
    return out


def _run(args):
    env = {k: v for k, v in os.environ.items() if k != "LD_PRELOAD"}
    env["ASAN_OPTIONS"] = "detect_leaks=1"
    r = subprocess.run([_build()] + [str(a) for a in args], env=env, capture_output=True, text=True)
    report = r.stdout[-2000:] + r.stderr[-6000:]
    assert r.returncode == 0, report
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, report
    return r.stdout, report


def test_schedule_and_record_order_properties(tmp_path):
    path = tmp_path / "cases.txt"
    path.write_text(cases.records_cases_text())
    out, report = _run([path])
    assert "match_schedule: ok (" in out and " 9 file cases" in out, report


def test_the_benchmark_run_has_ramps_of_three_steps_and_no_stub():
    out, _ = _run([499500, 31218, 1, 1024])
    sched = [tuple(map(int, line.split())) for line in out.splitlines()]
    sizes = [nb for _, nb in sched]
    assert sizes[:3] == [3902, 7804, 15609] and sizes[-3:] == [15609, 7804, 3902]
    assert len(sizes) == 21 and set(sizes[3:-3]) == {29658}
    assert [p0 for p0, _ in sched] == [sum(sizes[:k]) for k in range(21)] and sum(sizes) == 499500
