"""The tile kernel's block -> tile map (csrc/smvp_tile_map.h), forward and backward, checked on the host.

tests/tile_map_check.cpp is a program of its own: it includes the header -- which has no HIP in it -- and walks every grid the
library can launch for 1 ... 5000 tiles.  It is compiled here with the host compiler alone, under AddressSanitizer and
UndefinedBehaviorSanitizer (a toolchain without their runtimes compiles it plain: the checks are the program's own).  CPU only.
"""
import os
import shutil
import subprocess

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "tile_map_check.cpp")
INC = os.path.join(ROOT, "smvp-toolkit_amd", "csrc")


def compile_check(out, sanitize):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    # (the runtimes linked into the program itself: it then runs the same whatever else the process loads)
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-static-libasan",
           "-static-libubsan"] if sanitize else []
    return subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror"] + san + ["-I", INC, SRC, "-o", out],
                          capture_output=True, text=True)


def test_header_has_no_hip_in_it():
    text = open(os.path.join(INC, "smvp_tile_map.h")).read()
    assert "#include" not in text, "the host compiles smvp_tile_map.h alone: it includes nothing"


def test_tile_map_forward_and_backward(tmp_path):
    exe = str(tmp_path / "tile_map_check")
    p = compile_check(exe, True)
    sanitized = p.returncode == 0
    if not sanitized:
        assert ("cannot find" in p.stderr or "static-lib" in p.stderr) and ("asan" in p.stderr or "ubsan" in p.stderr), p.stderr[-3000:]
        p = compile_check(exe, False)
        assert p.returncode == 0, p.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stdout[-1500:] + r.stderr[-3000:]
    assert r.stdout.startswith("tile map ok: "), r.stdout[-1500:]
    print(r.stdout.strip(), "(under ASan + UBSan)" if sanitized else "(plain build: no sanitizer runtime here)")
