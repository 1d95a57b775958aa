"""CPU suite: the shared-memory link of a device group (gnark-whir_amd/csrc/group_link.h -- attach to a possibly stale segment, the chunk
rings, the all-gather area, the poison flag, the deadlines) as a program of its own: tests/cpp/group_link_host.cpp runs the ranks as
threads under the sanitizers.  The multi-process GPU tests (tests/test_gpu_group_multiprocess.py) run the same code under group.hip."""
import os
import subprocess
from gpu_common import ROOT


def test_the_link_under_the_sanitizers():
    """make sanitize-group-link: all-to-all batches around the ring's length, two transfers of one pair, a zero-byte transfer, 1000
    all-gathers with a lagging rank, the largest payload and one byte more, a rank that never enters (a timeout within 2 s, the link
    poisoned), a leftover segment under the group's name -- at worlds 2, 3 and 4, as a CPU build with AddressSanitizer and
    UndefinedBehaviorSanitizer, run as a program of its own"""
    src = os.path.join(ROOT, "gnark-whir_amd")
    r = subprocess.run(["make", "-C", src, "sanitize-group-link"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([os.path.join(src, "build", "group_link_host_asan")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "group link host: ok" in r.stdout, r.stdout + r.stderr
