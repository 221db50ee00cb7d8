"""Every path of the library gives back exactly what it took from the HIP runtime.

lib/libsmvp_amd_counted.so is the library's own objects linked with tests/resource_count.cpp: every HIP call by which the library
obtains or returns a resource -- device memory, pinned host memory, streams, events, graphs, graph execs -- is counted, and a
switch makes the nth obtaining call of a kind fail.  The scenarios live in tests/resource_scenarios.py and run in fresh child
processes that load the counted build through SMVP_LIB_PATH (this process keeps the plain one); every comparison there is exact
equality of counter snapshots.  Nothing here reads free-memory figures, so the tests do not depend on who else is on the card.

Out of scope: the RCCL communicators of the sharded layer (reached through dlopen()ed pointers, not through imported symbols),
and host-heap leaks (the host sources have their sanitizer programs, tests/test_host_sanitizers.py).

The groups run one after the other, each under its own time limit; nothing is retried, a child stops at its first failed
scenario, and once a child has crashed or run out of time no further group is started.
"""
import os
import subprocess
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

PKG = os.path.join(ROOT, "smvp-toolkit_amd")
COUNTED = os.path.join(PKG, "lib", "libsmvp_amd_counted.so")
SCRIPT = os.path.join(ROOT, "tests", "resource_scenarios.py")
GROUPS = ("csr", "tjds", "objects", "solvers", "sweep_csr", "sweep_tjds", "sweep_calls", "plan_bytes")
LIMIT_S = 240          # a group takes seconds; the limit only ends a child that hangs

_crashed = []


@pytest.fixture(scope="module")
def counted_library():
    if not os.path.exists(COUNTED):
        subprocess.check_call(["make", "-C", PKG, "lib/libsmvp_amd_counted.so"])
    return COUNTED


@pytest.mark.parametrize("group", GROUPS)
def test_every_path_gives_back_what_it_took(counted_library, group):
    assert not _crashed, "not started: the group %r ended in a crash or at its time limit" % _crashed[0]
    env = dict(os.environ, SMVP_LIB_PATH=counted_library)
    try:
        p = subprocess.run([sys.executable, SCRIPT, group], env=env, capture_output=True, text=True, timeout=LIMIT_S)
    except subprocess.TimeoutExpired as e:
        _crashed.append(group)
        raise AssertionError("group %s did not finish in %d s\n%s" % (group, LIMIT_S, (e.stdout or b"")[-3000:]))
    if p.returncode not in (0, 1, 2):
        _crashed.append(group)
    print(p.stdout[-6000:])
    assert p.returncode == 0 and ("group %s ok" % group) in p.stdout, \
        "group %s: exit status %d\n%s\n%s" % (group, p.returncode, p.stdout[-6000:], p.stderr[-3000:])
