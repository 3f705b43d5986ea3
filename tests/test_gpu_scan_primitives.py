"""The scan primitives of csrc/gtx_scan.h (wave_inclusive and its DPP form, tile_exclusive, run_exclusive_sum) on the device, at their
own seams rather than through whichever family happens to reach one: tests/tools/scan_check.hip instantiates them for blocks of 64, 256
and 1024 threads, at every n around a wave, a block and a load batch, and compares with plain host loops.  One child process."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECK = os.path.join(ROOT, "ibm-cbc-genomic-tools_amd", "csrc", "scan_check")


@pytest.mark.gpu
def test_scan_primitives_against_host_loops():
    assert os.path.exists(CHECK), "scan_check has not been built (make -C ibm-cbc-genomic-tools_amd/csrc)"
    r = subprocess.run([CHECK], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "scan_check ok" in r.stdout
