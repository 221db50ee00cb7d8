"""No result of the library depends on what the device memory it allocates for itself holds.

The suite controls every input of a product but one: the content of the library's own fresh allocations (plan buffers padded to a
tile, solver work spaces, timing rings, factor values).  A fresh process usually gets cleared pages, so a forgotten memset, a
padding slot that is summed or a partial folded before it is written gives the right answer in every other test and a wrong one
only in a long-lived process whose allocator hands back used memory.  lib/libsmvp_amd_counted.so routes every allocation of the
library through tests/resource_count.cpp, and smvp_test_fill_allocations fills each new block there before the library sees it:
every 32-bit word 0x00000001, or every byte 0xFF.  tests/fresh_memory_scenarios.py runs every path from scratch with the fill off
and under both patterns, in fresh child processes that load the counted build through SMVP_LIB_PATH (this process keeps the plain
one): each run is held to the check of the path's own GPU test, and all three must hand back the same bits.  Every group begins by
reading both patterns back from device memory byte for byte (smvp_test_probe_fill), so a fill that silently does nothing cannot
pass, and ends by requiring that fills were done and none failed.

A child's last lines say how many scenarios it ran and how long it took from its first import; on one MI355X (recorded in
profiles/fresh_memory_observed.txt): csr 8 s, csr_large 31 s, tjds 3 s, objects 3 s, solvers 20 s -- the longest uses an eighth of
LIMIT_S, which only ends a child that hangs.

The groups run one after the other, each under its own time limit; nothing is retried, a child stops at its first failed
scenario, and once a child has crashed or run out of time no further group is started.
"""
import os
import subprocess
import sys

import pytest

from conftest import ROOT
from test_gpu_resources import COUNTED, LIMIT_S, PKG

pytestmark = pytest.mark.gpu

SCRIPT = os.path.join(ROOT, "tests", "fresh_memory_scenarios.py")
GROUPS = ("csr", "csr_large", "tjds", "objects", "solvers")

_crashed = []


@pytest.fixture(scope="module")
def counted_library():
    if not os.path.exists(COUNTED):
        subprocess.check_call(["make", "-C", PKG, "lib/libsmvp_amd_counted.so"])
    return COUNTED


@pytest.mark.parametrize("group", GROUPS)
def test_no_result_depends_on_fresh_memory(counted_library, group):
    assert not _crashed, "not started: the group %r ended in a crash or at its time limit" % _crashed[0]
    env = dict(os.environ, SMVP_LIB_PATH=counted_library)
    try:
        p = subprocess.run([sys.executable, SCRIPT, group], env=env, capture_output=True, text=True, timeout=LIMIT_S)
    except subprocess.TimeoutExpired as e:
        _crashed.append(group)
        seen = e.stdout or ""                  # (what was captured up to a timeout comes as bytes on some Python versions)
        seen = seen.decode(errors="replace") if isinstance(seen, bytes) else seen
        raise AssertionError("group %s did not finish in %d s\n%s" % (group, LIMIT_S, seen[-3000:]))
    if p.returncode not in (0, 1, 2):
        _crashed.append(group)
    print(p.stdout[-6000:])
    assert p.returncode == 0 and ("group %s ok" % group) in p.stdout, \
        "group %s: exit status %d\n%s\n%s" % (group, p.returncode, p.stdout[-6000:], p.stderr[-3000:])
