"""GPU: what LSQR (smvp_csr_lsqr / smvp_tjds_lsqr, K22) takes it gives back, and it reads no memory it has not written --
tests/lsqr_scenarios.py in child processes on the counted library, as tests/test_gpu_gmres.py runs gmres_scenarios.py."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "smvp-toolkit_amd")
COUNTED = os.path.join(PKG, "lib", "libsmvp_amd_counted.so")
SCRIPT = os.path.join(ROOT, "tests", "lsqr_scenarios.py")
LIMIT_S = 240
_crashed = []


@pytest.mark.parametrize("group", ["resources", "fresh"])
def test_the_call_gives_back_what_it_took_and_reads_no_fresh_memory(group):
    """One child per group under one time limit, nothing retried: a successful call on either route, every refusal and each
    obtaining call failing in turn leave the counters where they were; the same solves under test_gpu_fresh_memory.py's fill
    patterns give the same bits.  After a child that crashed or ran into its limit nothing further is started."""
    assert not _crashed, "not started: the group %r ended in a crash or at its time limit" % _crashed[0]
    if not os.path.exists(COUNTED):
        subprocess.check_call(["make", "-C", PKG, "lib/libsmvp_amd_counted.so"])
    env = dict(os.environ, SMVP_LIB_PATH=COUNTED)
    try:
        p = subprocess.run([sys.executable, SCRIPT, group], env=env, capture_output=True, text=True, timeout=LIMIT_S)
    except subprocess.TimeoutExpired as e:
        _crashed.append(group)
        seen = e.stdout or ""
        seen = seen.decode(errors="replace") if isinstance(seen, bytes) else seen
        raise AssertionError("group %s did not finish in %d s\n%s" % (group, LIMIT_S, seen[-3000:]))
    if p.returncode not in (0, 1, 2):
        _crashed.append(group)
    print(p.stdout[-6000:])
    assert p.returncode == 0 and ("group %s ok" % group) in p.stdout, \
        "group %s: exit status %d\n%s\n%s" % (group, p.returncode, p.stdout[-6000:], p.stderr[-3000:])
