"""CPU check of lane_slam_amd/csrc/nfa.h, the one NFA routine of both line detectors: compiled for the host
(tests/hostsim/nfa_host.cpp, g++ with -ffp-contract=off as the hostsim fixture), each of its two forms must give the bits
of its own detector's oracle -- log_gamma(n + 1) as the first term against the EDLines oracle, n + 1 itself against the
LSD oracle -- over a grid that reaches every branch of the routine."""
import ctypes
import itertools
import os
import struct
import subprocess

import pytest

from oracle import oracle as O

HERE = os.path.dirname(os.path.abspath(__file__))
PS = (0.125, 0.0625, 0.03125)            # LSD's p = ang_th / 180 and its two halvings; EDLines uses 0.125 only
LOG_NTS = (11.5, 7.0)


@pytest.fixture(scope="module")
def nfa_host():
    so = os.path.join(HERE, "hostsim", "_build", "libnfahost.so")
    src = os.path.join(HERE, "hostsim", "nfa_host.cpp")
    hdrs = [os.path.join(HERE, "..", "lane_slam_amd", "csrc", h) for h in ("nfa.h", "detmath.h")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(f) for f in [src] + hdrs):
        os.makedirs(os.path.dirname(so), exist_ok=True)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-o", so, src])
    lib = ctypes.CDLL(so)
    for f in (lib.nfa_log_gamma_first, lib.nfa_plain_first):
        f.restype = ctypes.c_double
        f.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_double]
    return lib


def _grid():
    """(n, k) pairs: the two early exits, n + 1 / k + 1 / n - k + 1 on both sides of the log-gamma switch at 15, and the
    three named branches of the tail."""
    small = range(0, 20)                                           # n == 0, k == 0, n == k, and 13 .. 17 around the switch
    nk = {(n, k) for n, k in itertools.product(small, small) if k <= n}
    nk |= {(n, k) for n in (28, 29, 30, 31, 32, 33) for k in (1, 13, 14, 15, 16, 17) if k <= n}      # n - k + 1 around 15 with n + 1 above it
    nk |= {(20000, 10000), (20000, 100), (5000, 700), (5000, 0), (0, 0), (700, 700), (300, 60), (1000, 125), (1000, 126), (4096, 512)}
    return sorted(nk)


def _bits(v):
    return struct.pack("<d", v)


@pytest.mark.parametrize("form", ["log_gamma_first", "plain_first"])
def test_nfa_matches_its_oracle_bit_for_bit(nfa_host, form):
    mine = nfa_host.nfa_log_gamma_first if form == "log_gamma_first" else nfa_host.nfa_plain_first
    ref = O.ed_nfa if form == "log_gamma_first" else O.lsd_nfa
    n_cases = 0
    for (n, k), p, log_nt in itertools.product(_grid(), PS, LOG_NTS):
        a, b = mine(n, k, p, log_nt), ref(n, k, p, log_nt)
        assert _bits(a) == _bits(b), (form, n, k, p, log_nt, a, b)
        n_cases += 1
    assert n_cases > 1000


def test_nfa_named_branches(nfa_host):
    """Known values on the branches the grid is there for, so that it is known to reach them: the underflow branch with
    k > n p and with k <= n p, both early exits, and a tail that stops early (it differs from the full sum's exit only in
    time, so it is pinned by the oracle's bits above)."""
    f = nfa_host.nfa_log_gamma_first
    assert f(20000, 10000, 0.125, 11.5) == 3580.9680067817094          # exp(log1term) == 0, k > n p: -log1term / ln 10 - log_nt
    assert f(20000, 100, 0.125, 11.5) == -11.5                         # exp(log1term) == 0, k <= n p
    assert f(0, 5, 0.125, 11.5) == -11.5 and f(5, 0, 0.125, 11.5) == -11.5
    assert f(16, 16, 0.125, 11.5) == O.ed_nfa(16, 16, 0.125, 11.5) != -11.5      # n == k
    import math
    assert math.isfinite(f(5000, 700, 0.125, 11.5))


def test_the_two_forms_differ_where_they_should(nfa_host):
    """The first-term difference is real: the forms agree on the exits that never reach it and differ in the tail."""
    a, b = nfa_host.nfa_log_gamma_first, nfa_host.nfa_plain_first
    assert a(0, 0, 0.125, 11.5) == b(0, 0, 0.125, 11.5)
    assert a(16, 16, 0.125, 11.5) == b(16, 16, 0.125, 11.5)
    assert a(300, 60, 0.125, 11.5) != b(300, 60, 0.125, 11.5)
