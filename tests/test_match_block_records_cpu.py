"""CPU: the block-granular record builder alone (openmvg_amd/csrc/mvgx_match_batch.h, plain C++ without HIP).

tests/native/match_records_main.cpp is a stand-alone program (its own main, AddressSanitizer and UndefinedBehaviorSanitizer linked in: no
preloaded runtime). It runs the builder over the pair lists of tests/_match_block_cases.py, whole and in batches of 3 and 8 pairs, and over
random image sets and lists of its own, into buffers of exactly the size the matcher reserves, decodes the records as the kernels do and
asserts what its header lists. Pass = exit status 0, its last line, and no sanitizer report."""
import os
import subprocess

from tests import _emu, _match_block_cases as cases

_NATIVE = os.path.join(_emu._HERE, "native")
_MAIN = os.path.join(_NATIVE, "match_records_main.cpp")
_HEADER = os.path.join(_emu._ROOT, "openmvg_amd", "csrc", "mvgx_match_batch.h")


def _build():
    out = os.path.join(_NATIVE, "_build", "match_records")
    if os.path.exists(out) and all(os.path.getmtime(d) <= os.path.getmtime(out) for d in (_MAIN, _HEADER)):
        return out
    os.makedirs(os.path.dirname(out), exist_ok=True)
    cxx = _emu._CLANG if os.path.exists(_emu._CLANG) else "clang++"
    subprocess.run([cxx, "-x", "c++", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                    "-g", "-O1", "-Wall", "-Werror", "-I" + os.path.dirname(_HEADER), _MAIN, "-o", out], check=True)
    return out


def test_builder_covers_every_block_once(tmp_path):
    exe = _build()
    path = tmp_path / "cases.txt"
    path.write_text(cases.records_cases_text())
    env = {k: v for k, v in os.environ.items() if k != "LD_PRELOAD"}
    env["ASAN_OPTIONS"] = "detect_leaks=1"
    r = subprocess.run([exe, str(path)], env=env, capture_output=True, text=True)
    report = r.stdout[-2000:] + r.stderr[-6000:]
    assert r.returncode == 0, report
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, report
    assert "match_records: ok (9 file cases" in r.stdout, report
