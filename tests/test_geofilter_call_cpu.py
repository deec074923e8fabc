"""CPU: the host path of a geometric-filter call under AddressSanitizer and UndefinedBehaviorSanitizer.

tests/native/geofilter_call_main.cpp is a stand-alone program (its own main, the sanitizers linked in: no preloaded runtime) over the HIP
emulation of openmvg_amd/csrc/mvgx_geofilter.hip. It calls all ten mvgx_geofilter_* entries on pairs of 0 / a minimal sample / one more /
24 correspondences, compares the indexed entries with the gathered ones and the global-table form with the LDS form byte for byte, makes
the calls without work (no pair, only pairs below a minimal sample), and walks the emulation's allocation-failure injection through every
allocation of a gathered and of an indexed call. Pass = exit status 0, the program's "ok" line and no sanitizer report.
"""
import os
import subprocess

from tests import _emu

_NATIVE = os.path.join(_emu._HERE, "native")
_MAIN = os.path.join(_NATIVE, "geofilter_call_main.cpp")


def _build():
    out = os.path.join(_NATIVE, "_build", "geofilter_call")
    csrc = os.path.join(_emu._ROOT, "openmvg_amd", "csrc")
    deps = [_MAIN, os.path.join(_emu._SRC, "hipemu.cpp"), os.path.join(_emu._SRC, "hip", "hip_runtime.h"), os.path.join(_emu._ROOT, "include", "mvgx.h")]
    deps += [os.path.join(csrc, f) for f in os.listdir(csrc)]
    if os.path.exists(out) and all(os.path.getmtime(d) <= os.path.getmtime(out) for d in deps):
        return out
    os.makedirs(os.path.dirname(out), exist_ok=True)
    cxx = _emu._CLANG if os.path.exists(_emu._CLANG) else "clang++"
    subprocess.run([cxx, "-x", "c++", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize=vptr,function", "-fno-omit-frame-pointer", "-g", "-O1",
                    "-Wno-psabi", "-I" + _emu._SRC, "-I" + os.path.join(_emu._ROOT, "include"), "-I" + csrc, _MAIN, "-o", out], check=True)
    return out


def test_every_entry_and_every_failing_allocation_under_the_sanitizers():
    exe = _build()
    env = {k: v for k, v in os.environ.items() if k not in ("LD_PRELOAD", "HIPEMU_FAIL_MALLOC_AFTER")}
    env["ASAN_OPTIONS"] = "detect_leaks=1"
    env["UBSAN_OPTIONS"] = "print_stacktrace=1"
    r = subprocess.run([exe], env=env, capture_output=True, text=True)
    report = r.stdout[-2000:] + r.stderr[-6000:]
    assert r.returncode == 0, report
    assert "AddressSanitizer" not in r.stderr and "LeakSanitizer" not in r.stderr and "runtime error" not in r.stderr, report
    assert "geofilter_call: ok" in r.stdout
