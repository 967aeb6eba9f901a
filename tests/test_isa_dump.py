"""tools/isa_dump.py --compare: the device-code check of a host-side change
(no GPU: it disassembles the objects the build left in the tree)."""
import os
import subprocess
import sys

from conftest import ROOT

TOOL = os.path.join(ROOT, "tools", "isa_dump.py")
CSRC = os.path.join(ROOT, "qkd_ldpc_v_amd", "csrc")


def _compare(a, b):
    return subprocess.run([sys.executable, TOOL, "--compare", os.path.join(CSRC, a), os.path.join(CSRC, b)],
                          capture_output=True, text=True)


def test_compare_accepts_an_object_against_itself():
    r = _compare("order.o", "order.o")
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 in one file only, 0 differing" in r.stdout


def test_compare_reports_missing_symbols_and_fails():
    r = _compare("order.o", "trials.o")
    assert r.returncode == 1, r.stdout + r.stderr
    assert "frame_order_kernel" in r.stdout and "only in" in r.stdout
