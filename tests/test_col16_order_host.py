"""Where the plan keeps the 16-bit column offsets of a full, narrow tile (csrc/smvp_tile_map.h, col16_slot), checked on the host.

tests/col16_order_check.cpp is a program of its own: it includes the header -- which has no HIP in it -- and checks, for tiles of
1024 and 2048 entries, that the slot function is a bijection of the tile that stays inside every wavefront's chunk, and that the
entries of a lane (tile_lane_entry) have consecutive slots in the lane's own order, at the address the kernel loads from.  It is
compiled here with the host compiler alone, under AddressSanitizer and UndefinedBehaviorSanitizer (a toolchain without their
runtimes compiles it plain: the checks are the program's own).  CPU only.
"""
import os
import shutil
import subprocess

from conftest import ROOT
from tile_layout import lane_entry

SRC = os.path.join(ROOT, "tests", "col16_order_check.cpp")
INC = os.path.join(ROOT, "smvp-toolkit_amd", "csrc")


def compile_check(out, sanitize):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    # (the runtimes linked into the program itself: it then runs the same whatever else the process loads)
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-static-libasan",
           "-static-libubsan"] if sanitize else []
    return subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror"] + san + ["-I", INC, SRC, "-o", out],
                          capture_output=True, text=True)


def test_col16_slot_on_the_host(tmp_path):
    exe = str(tmp_path / "col16_order_check")
    p = compile_check(exe, True)
    sanitized = p.returncode == 0
    if not sanitized:
        assert ("cannot find" in p.stderr or "static-lib" in p.stderr) and ("asan" in p.stderr or "ubsan" in p.stderr), p.stderr[-3000:]
        p = compile_check(exe, False)
        assert p.returncode == 0, p.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stdout[-1500:] + r.stderr[-3000:]
    assert r.stdout.startswith("col16 order ok: 3072 "), r.stdout[-1500:]
    print(r.stdout.strip(), "(under ASan + UBSan)" if sanitized else "(plain build: no sanitizer runtime here)")


def test_python_mirror_of_the_slot():
    """tile_layout.lane_entry (the tests' hand copy of the kernel's formula) against the slot formula written out in Python:
    the structure test_gpu_col16_order.py builds relies on chunks of 64 * VPT entries, which is all it takes from here."""
    for vpt in (4, 8):
        slots = set()
        for t in range(256):
            for k in range(vpt):
                o = lane_entry(vpt, t, k)
                q = o % (64 * vpt)
                slot = (o // (64 * vpt)) * 64 * vpt + ((q % 128) // 2) * vpt + 2 * (q // 128) + (q & 1)
                assert slot == (t >> 6) * 64 * vpt + (t & 63) * vpt + k
                slots.add(slot)
        assert slots == set(range(256 * vpt))
