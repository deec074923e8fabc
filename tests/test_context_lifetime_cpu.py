"""CPU: the matcher contexts own their memory - nothing leaks, nothing is freed twice, also when an allocation fails half-way.

tests/native/context_lifetime_main.cpp is a stand-alone program (its own main, AddressSanitizer linked in: no preloaded runtime) over the
HIP emulation of the product's matching sources. It drives every context kind through the C ABI - create, regions of 0 / 5 / 70
descriptors, all ordered pairs in two or more batches, regions of 0 / 130 / 70 descriptors so that the buffers regrow, the pairs again,
destroy - then repeats each sequence with the emulation's allocation-failure injection at the first allocation, at one inside set_regions
and at one inside run, and checks that mvgx_match_run_stream with "stream_hold" hands out, and the context frees, both sets of host
buffers. One program per emulation source (the two define the same symbols): mvgx_match_* from hipemu_match.cpp, the Hamming / L2-float /
L2-uint8 / cascade contexts from hipemu.cpp. Pass = exit status 0 and no AddressSanitizer or LeakSanitizer report.
"""
import os
import subprocess

import pytest

from tests import _emu

_NATIVE = os.path.join(_emu._HERE, "native")
_MAIN = os.path.join(_NATIVE, "context_lifetime_main.cpp")


def _build(which):
    out = os.path.join(_NATIVE, "_build", "context_lifetime_" + which)
    csrc = os.path.join(_emu._ROOT, "openmvg_amd", "csrc")
    gen = _emu.generate_match_source()
    deps = [_MAIN, gen, os.path.join(_emu._SRC, "hipemu.cpp"), os.path.join(_emu._SRC, "hipemu_match.cpp"),
            os.path.join(_emu._SRC, "hip", "hip_runtime.h"), os.path.join(_emu._ROOT, "include", "mvgx.h")]
    deps += [os.path.join(csrc, f) for f in os.listdir(csrc)]
    if os.path.exists(out) and all(os.path.getmtime(d) <= os.path.getmtime(out) for d in deps):
        return out
    cxx = _emu._CLANG if os.path.exists(_emu._CLANG) else "clang++"
    subprocess.run([cxx, "-x", "c++", "-std=c++17", "-fsanitize=address", "-fno-omit-frame-pointer", "-g", "-O1", "-Wno-psabi",
                    *(["-DLIFETIME_MATCH"] if which == "match" else []), "-I" + _emu._SRC, "-I" + os.path.dirname(gen),
                    "-I" + os.path.join(_emu._ROOT, "include"), "-I" + csrc, _MAIN, "-o", out], check=True)
    return out


@pytest.mark.parametrize("which", ["match", "bruteforce"])
def test_contexts_free_what_they_own(which):
    exe = _build(which)
    env = {k: v for k, v in os.environ.items() if k not in ("LD_PRELOAD", "HIPEMU_FAIL_MALLOC_AFTER")}
    env["ASAN_OPTIONS"] = "detect_leaks=1"
    r = subprocess.run([exe], env=env, capture_output=True, text=True)
    report = r.stdout[-2000:] + r.stderr[-6000:]
    assert r.returncode == 0, report
    assert "AddressSanitizer" not in r.stderr and "LeakSanitizer" not in r.stderr, report
    assert "context_lifetime: ok" in r.stdout
