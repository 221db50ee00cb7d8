"""The counted build of the library (tests/resource_count.cpp, lib/libsmvp_amd_counted.so) as far as a machine without a GPU can
check it: the bookkeeping under AddressSanitizer + UndefinedBehaviorSanitizer over a fake runtime, the list of wrapped HIP calls
against what the library really imports, and the two libraries' exported entry points.  tests/test_gpu_resources.py uses it on
the GPU.  CPU only.
"""
import os
import re
import shutil
import subprocess

import pytest

import smvp_toolkit_amd as sm
from conftest import ROOT

PKG = os.path.join(ROOT, "smvp-toolkit_amd")
PLAIN = os.path.join(PKG, "lib", "libsmvp_amd.so")
COUNTED = os.path.join(PKG, "lib", "libsmvp_amd_counted.so")
CHECK = os.path.join(PKG, "build", "san", "resource_count_check")
OBTAINS = re.compile(r"^hip.*(Malloc|Alloc|Create|Instantiate|EndCapture)")
TEST_EXPORTS = {"smvp_test_resources", "smvp_test_fail_device_alloc", "smvp_test_fail_host_alloc", "smvp_test_fail_stream_create",
                "smvp_test_fail_event_create", "smvp_test_fill_allocations", "smvp_test_fill_stats", "smvp_test_probe_fill"}


def nm(*args):
    tool = shutil.which("nm") or shutil.which("llvm-nm") or "/opt/rocm/lib/llvm/bin/llvm-nm"
    return subprocess.run([tool] + list(args), check=True, capture_output=True, text=True).stdout


def symbols(path, which):
    """Names of the dynamic symbols `path` defines ("--defined-only") or imports ("--undefined-only"), versions cut off."""
    return {line.split()[-1].split("@")[0] for line in nm("-D", which, path).splitlines() if line.strip()}


@pytest.fixture(scope="module")
def libraries():
    if not (os.path.exists(PLAIN) and os.path.exists(COUNTED)):
        subprocess.check_call(["make", "-C", PKG, "lib/libsmvp_amd.so", "lib/libsmvp_amd_counted.so"])
    return PLAIN, COUNTED


def wrapped_calls():
    return set(subprocess.run(["make", "-s", "-C", PKG, "print-counted-wraps"], check=True, capture_output=True, text=True).stdout.split())


def test_the_bookkeeping_under_asan_and_ubsan():
    """Balance, bytes, foreign frees, the nth-failure switches and re-arming, from eight threads: a stand-alone program with
    its own main, run as its own process like the host-san programs."""
    p = subprocess.run(["make", "-C", PKG, "resource-check"], capture_output=True, text=True)
    if p.returncode != 0:
        if "cannot find" in p.stderr and ("asan" in p.stderr or "ubsan" in p.stderr):
            pytest.skip("this toolchain has no sanitizer runtime: " + p.stderr[-300:])
        raise AssertionError(p.stderr[-3000:])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    p = subprocess.run([CHECK], capture_output=True, text=True, env=env, timeout=300)
    assert p.returncode == 0 and "resource_count_check ok" in p.stdout and "Sanitizer" not in p.stderr and "runtime error" not in p.stderr, \
        "%s\n%s" % (p.stdout[-1500:], p.stderr[-4000:])


def test_every_obtaining_hip_call_the_library_imports_is_wrapped(libraries):
    """A hipMallocAsync or hipExtMallocWithFlags that csrc/ starts to call fails this test until the Makefile wraps it and
    tests/resource_count.cpp counts it."""
    plain, _ = libraries
    imported = {s for s in symbols(plain, "--undefined-only") if OBTAINS.match(s)}
    wrapped = wrapped_calls()
    assert imported, "libsmvp_amd.so imports no allocating HIP call: the symbol listing is broken"
    assert imported <= wrapped, "not counted by the counted build: %s" % sorted(imported - wrapped)
    # ... and every wrapped call has its wrapper in the unit (the link would fail without it) and its releasing partner
    unit = open(os.path.join(ROOT, "tests", "resource_count.cpp")).read()
    for name in wrapped:
        assert "__wrap_%s(" % name in unit and "__real_%s(" % name in unit, name
    for release in ("hipFree", "hipHostFree", "hipStreamDestroy", "hipEventDestroy", "hipGraphDestroy", "hipGraphExecDestroy"):
        assert release in wrapped, release


def test_the_obtaining_pattern_knows_its_calls():
    for name in ("hipMalloc", "hipMallocAsync", "hipExtMallocWithFlags", "hipHostMalloc", "hipHostAlloc", "hipStreamCreateWithPriority",
                 "hipEventCreateWithFlags", "hipGraphInstantiate", "hipStreamEndCapture", "hipMemPoolCreate", "hipMallocPitch"):
        assert OBTAINS.match(name), name
    for name in ("hipFree", "hipMemcpy", "hipLaunchKernel", "hipStreamSynchronize", "hipGraphLaunch"):
        assert not OBTAINS.match(name), name


def test_the_two_libraries_export_the_same_entry_points(libraries):
    plain, counted = libraries
    mine = {s for s in symbols(plain, "--defined-only") if s.startswith("smvp_")}
    theirs = {s for s in symbols(counted, "--defined-only") if s.startswith("smvp_")}
    assert set(sm.EXPORTS) <= mine
    assert theirs - mine == TEST_EXPORTS and mine - theirs == set()
    assert not any(s.startswith("smvp_test_") for s in mine), "the test switches leaked into libsmvp_amd.so"
    # the wrappers themselves stay inside the counted library: nobody else's hipMalloc may bind to them
    assert not any(s.startswith("__wrap_") or s.startswith("__real_") for s in symbols(counted, "--defined-only"))
    # the counted library reaches the runtime for every wrapped call (through __real_), the plain one as before
    assert wrapped_calls() <= symbols(counted, "--undefined-only")
