"""CPU suite: peakdiff's tables of critical counts (csrc/gtx_peakdiff.h through the host-only `gtx_packtool critical`) against the
tail evaluated directly.  The builder finds kcrit[c] by bisection over k, which takes the computed tail not to rise with k; the
computed tail changes sides at the mean, so that is checked here and not trusted: for EVERY (k, c) in [0, W]^2 the table's answer
k >= kcrit[c] must equal orc_binomial_Q(k, p(c), W) <= cutoff."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from oracle import orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PACKTOOL = os.path.join(ROOT, "ibm-cbc-genomic-tools_amd", "csrc", "gtx_packtool")

WS = [1, 5, 20, 100, 500]
BACKGROUNDS = [1e-6, 1e-3, 0.02, 0.3]
CUTOFFS = [0.0, 1e-5, 0.05, 1.0]


def critical(p, W, cutoff, control):
    r = subprocess.run([PACKTOOL, "critical", "%.17g" % p, str(W), "%.17g" % cutoff, "1" if control else "0"], capture_output=True)
    assert r.returncode == 0, r.stderr.decode()
    return np.array([int(x) for x in r.stdout.split()], dtype=np.int64)


@pytest.fixture(scope="module")
def Q():
    L = orc.lib()
    L.orc_binomial_Q.restype = ctypes.c_double
    L.orc_binomial_Q.argtypes = [ctypes.c_long, ctypes.c_double, ctypes.c_long]
    return L.orc_binomial_Q


@pytest.mark.parametrize("W", WS)
def test_tables_equal_the_direct_tail_for_every_count_pair(Q, W):
    for p0 in BACKGROUNDS:
        # the tail per (c, k), once for all cutoffs
        tail = np.array([[Q(k, max(p0, min(c / W, 1.0)), W) for k in range(W + 1)] for c in range(W + 1)])
        for cutoff in CUTOFFS:
            kcrit = critical(p0, W, cutoff, True)
            assert kcrit.shape == (W + 1,) and kcrit.min() >= 0 and kcrit.max() <= W + 1
            got = np.arange(W + 1)[None, :] >= kcrit[:, None]
            want = tail <= cutoff
            bad = np.argwhere(got != want)
            assert bad.size == 0, "W=%d p=%g cutoff=%g: first (c, k) that differs %s" % (W, p0, cutoff, bad[0].tolist())
            one = critical(p0, W, cutoff, False)
            assert one.shape == (1,) and one[0] == kcrit[0]          # c = 0: p = the background


def test_no_count_passes_a_negative_cutoff():
    assert critical(0.02, 20, -1.0, True).tolist() == [21] * 21


def test_usage():
    r = subprocess.run([PACKTOOL, "critical", "0.1"], capture_output=True)
    assert r.returncode == 2 and b"usage: gtx_packtool critical" in r.stderr
