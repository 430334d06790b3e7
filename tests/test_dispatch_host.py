"""csrc/knp_dispatch.hpp on the host alone (no GPU): tools/dispatch_check.cpp runs with_lanes / clamp_lanes over the four <LO, HI> ranges
the launchers use and every lane count from -2 to 130, and with_flag / with_either on both values; the rule is restated here."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RANGES = [(2, 16), (2, 32), (2, 64), (4, 32)]
LANES = range(-2, 131)


def _rule(lo, hi, n):
    """A power of two in [lo, hi) runs its own instantiation, every other count the widest one."""
    return n if n in [2 ** k for k in range(8)] and lo <= n < hi else hi


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    probe = subprocess.run("echo 'int main(){return 0;}' | g++ -x c++ -fsanitize=address,undefined - -o /dev/null", shell=True, capture_output=True)
    san = ["-fsanitize=address,undefined", "-fno-omit-frame-pointer"] if probe.returncode == 0 else []
    exe = str(tmp_path_factory.mktemp("dispatch") / "dispatch_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror"] + san + ["-I" + os.path.join(ROOT, "knp-emi-cgx_amd", "csrc"),
                    os.path.join(ROOT, "tools", "dispatch_check.cpp"), "-o", exe], check=True, capture_output=True, text=True, timeout=120)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    return [ln.split() for ln in r.stdout.splitlines()]


def test_with_lanes_calls_once_with_the_clamped_width(lines):
    seen = {}
    for ln in lines:
        if ln[0] == "lanes":
            lo, hi, n, calls, got, clamp = map(int, ln[1:])
            assert (lo, hi, n) not in seen
            seen[(lo, hi, n)] = (calls, got, clamp)
    assert sorted(seen) == sorted((lo, hi, n) for lo, hi in RANGES for n in LANES)
    for (lo, hi, n), (calls, got, clamp) in seen.items():
        want = _rule(lo, hi, n)
        assert calls == 1, (lo, hi, n, calls)
        assert got == want, (lo, hi, n, got, want)
        assert clamp == want, (lo, hi, n, clamp, want)


def test_with_flag_and_with_either_take_the_matching_branch_once(lines):
    flag = {int(ln[1]): (int(ln[2]), int(ln[3])) for ln in lines if ln[0] == "flag"}
    assert flag == {0: (0, 1), 1: (1, 0)}
    either = {tuple(map(int, ln[1:4])): (int(ln[4]), int(ln[5])) for ln in lines if ln[0] == "either"}
    assert either == {(a, b, first): (1, a if first else b) for a, b in [(1, 2), (2, 3), (3, 8)] for first in (0, 1)}
