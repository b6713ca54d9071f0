"""plan_merkle (csrc/merkle_plan.h): which Merkle path launch_merkle tries, in what order and with what launch
geometry, pinned on the host.  Every path writes the same output vector, so a slip in a condition would only
make a root slower, which no GPU parity test notices.  The expected plans were derived by hand from the
launchers this function replaced, for a device of 256 compute units."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K, S = 0, 1  # Keccak256, SM3
CUS = 256

# (hasher, width, n, switches) in the order of CASES below
CASES = {
    "k_w2_10k": (K, 2, 10_000, ""),
    "k_w16_100k": (K, 16, 100_000, ""),
    "s_w16_100k": (S, 16, 100_000, ""),
    "s_w16_100k_sm3climb": (S, 16, 100_000, "SM3CLIMB=1"),
    "s_w2_10k": (S, 2, 10_000, ""),
    "k_w16_16m": (K, 16, 1 << 24, ""),
    "s_w16_16m": (S, 16, 1 << 24, ""),
    "k_w16_16m_nosub": (K, 16, 1 << 24, "NOSUB=1"),
    "s_w16_16m_nosub": (S, 16, 1 << 24, "NOSUB=1"),
    "k_w16_16m_nosub_lat": (K, 16, 1 << 24, "NOSUB=1,LATSCHED=1"),
    "s_w16_16m_nosub_lat": (S, 16, 1 << 24, "NOSUB=1,LATSCHED=1"),
    "k_w2_16m": (K, 2, 1 << 24, ""),
    "k_w2_1m": (K, 2, 1_000_000, ""),
    "k_w64_100k": (K, 64, 100_000, ""),
    "k_w2_10k_twolaunch": (K, 2, 10_000, "CLIMB=0,FUSED=0"),
    "k_w2_10k_levelwise": (K, 2, 10_000, "LEVELWISE=1"),
    "s_w16_16m_levelwise": (S, 16, 1 << 24, "LEVELWISE=1,CLIMB=1,FUSED=1"),
    "n0": (K, 2, 0, ""),
    "w1": (S, 1, 100, "CLIMB=1"),
    "w65": (K, 65, 100, "LEVELWISE=1"),
    "n1": (K, 2, 1, ""),
    "n1_levelwise": (S, 16, 1, "LEVELWISE=1"),
    "n1_fused": (S, 64, 1, "FUSED=1"),
    # the static limits: a forced path that cannot run is not listed
    "k_w16_256m_climb_nosub": (K, 16, 1 << 28, "CLIMB=1,NOSUB=1"),  # 65,536 workgroups > kClimbMaxWgs
    "k_w2_16m_fused": (K, 2, 1 << 24, "FUSED=1"),                   # 262,143 counters > kFusedCounters
    "s_w16_100k_fused": (S, 16, 100_000, "FUSED=1"),                # forced on for SM3
    "k_w16_1m": (K, 16, 1_000_000, ""),                            # 3,907 waves > kFusedMaxWaves, not forced
    # which values count as set
    "parse_a": (K, 2, 10_000, "LEVELWISE=01,FUSED=2,CLIMB=1x,SM3CLIMB=10,PAIR=00,SM3X=yes,NOSUB=0,LATSCHED=11"),
    "parse_b": (K, 2, 10_000, "LEVELWISE=10,FUSED=,CLIMB=-1,SM3CLIMB=true,PAIR=1,SM3X=0,NOSUB=1,LATSCHED=01"),
}


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("g++ not found")
    exe = str(tmp_path_factory.mktemp("merkle_plan") / "merkle_plan_test")
    subprocess.run([cxx, "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-o", exe,
                    os.path.join(ROOT, "tests", "cpp", "merkle_plan_test.cpp")], check=True)
    args = ["%d:%d:%d:%d:%s" % (h, w, n, CUS, sw) for h, w, n, sw in CASES.values()]
    r = subprocess.run([exe] + args, check=True, capture_output=True, text=True)
    lines = r.stdout.splitlines()
    assert len(lines) == len(CASES)
    return dict(zip(CASES, (json.loads(x) for x in lines)))


def _sub(d, **want):
    got = {k: d[k] for k in want}
    assert got == want


def test_keccak_w2_latency_climbs(plans):
    p = plans["k_w2_10k"]
    assert p["kind"] == "tree" and p["nlev"] == 14
    assert p["paths"] == ["climb", "fused", "two_launch"]
    _sub(p["climb"], k=-1, wgs=20, latency=1, coop_max=8, pair_max=128, B=256, kin=8, g=4, counters=21, x=0, pair=1)
    _sub(p["climb"]["t"], nlev=14, cnt0=5000, pos0=0)
    _sub(p["fused"], S=32, a=5, grid=157, counters=160)


def test_keccak_w16_latency_is_fused(plans):
    p = plans["k_w16_100k"]
    assert p["paths"] == ["fused", "two_launch"]
    _sub(p["fused"], S=16, a=1, grid=391, counters=28)
    _sub(p["two_launch"], B=256, kin=2, grid=25, pair=1, threads=512, sm3x=0, sm3x_top=0, nmid=0, top=3)


def test_sm3_w16_latency_is_two_launch(plans):
    p = plans["s_w16_100k"]
    assert p["paths"] == ["two_launch"]
    _sub(p["two_launch"], B=256, kin=2, grid=25, threads=256, pair=0, sm3x=1, sm3x_top=1, nmid=0, top=3)


def test_sm3_climb_opt_in(plans):
    p = plans["s_w16_100k_sm3climb"]
    assert p["paths"] == ["climb", "two_launch"]
    _sub(p["climb"], k=-1, x=1, wgs=25, g=2, latency=1, B=256, kin=2)


def test_sm3_w2_two_launch(plans):
    p = plans["s_w2_10k"]
    assert p["paths"] == ["two_launch"]
    _sub(p["two_launch"], grid=20, sm3x=1, sm3x_top=1, top=9, nmid=0, kin=8, B=256, threads=256, pair=0)


@pytest.mark.parametrize("name,g", [("k_w16_16m", 1), ("s_w16_16m", 2)])
def test_w16_throughput_subtree_then_climb(plans, name, g):
    p = plans[name]
    assert p["paths"] == ["climb", "two_launch"]
    _sub(p["climb"], k=0, sub_grid=4096, wgs=256, latency=1, coop_max=8, pair_max=128, counters=17, g=g, x=0)
    _sub(p["climb"]["t"], nlev=5, cnt0=65536, pos0=(1 << 20) + 1)


@pytest.mark.parametrize("name", ["k_w16_16m_nosub", "s_w16_16m_nosub"])
def test_nosub_throughput_schedule(plans, name):
    p = plans[name]
    assert p["paths"][0] == "climb"
    _sub(p["climb"], k=-1, wgs=4096, latency=0, coop_max=2, pair_max=32, counters=273)
    _sub(p["climb"]["t"], nlev=6, cnt0=1 << 20, pos0=0)


@pytest.mark.parametrize("name", ["k_w16_16m_nosub_lat", "s_w16_16m_nosub_lat"])
def test_nosub_latsched(plans, name):
    p = plans[name]
    assert p["paths"][0] == "climb"
    _sub(p["climb"], k=-1, wgs=4096, latency=1, coop_max=8, pair_max=128, counters=273)


def test_keccak_w2_throughput_subtree_depth(plans):
    p = plans["k_w2_16m"]
    assert p["paths"] == ["climb", "two_launch"]
    _sub(p["climb"], k=6, sub_grid=512, wgs=256, counters=255, latency=1, g=4)
    _sub(p["climb"]["t"], nlev=17, cnt0=1 << 16)
    p = plans["k_w2_1m"]
    _sub(p["climb"], k=2, wgs=245, latency=1)
    assert p["paths"][0] == "climb"


def test_keccak_w64_fused_one_node_per_wave(plans):
    p = plans["k_w64_100k"]
    assert p["paths"] == ["fused", "two_launch"]
    _sub(p["fused"], S=1, a=0, grid=1563)


def test_forced_two_launch(plans):
    p = plans["k_w2_10k_twolaunch"]
    assert p["paths"] == ["two_launch"]
    _sub(p["two_launch"], pair=1, threads=512, B=256, kin=8, grid=20, top=9)


def test_levelwise_alone(plans):
    for name, nlev in (("k_w2_10k_levelwise", 14), ("s_w16_16m_levelwise", 6)):
        assert plans[name]["paths"] == ["levelwise"] and plans[name]["kind"] == "tree"
        assert plans[name]["nlev"] == nlev


def test_argument_errors_and_copy(plans):
    for name in ("n0", "w1", "w65"):
        assert plans[name]["kind"] == "arg_error" and plans[name]["paths"] == []
    for name in ("n1", "n1_levelwise", "n1_fused"):
        assert plans[name]["kind"] == "copy" and plans[name]["paths"] == []


def test_static_limits(plans):
    assert plans["k_w16_256m_climb_nosub"]["paths"] == ["two_launch"]
    _sub(plans["k_w16_256m_climb_nosub"]["two_launch"], grid=65536, pair=0, threads=512, nmid=1, top=4)
    assert plans["k_w2_16m_fused"]["paths"] == ["two_launch"]
    assert plans["s_w16_100k_fused"]["paths"] == ["fused", "two_launch"]
    _sub(plans["s_w16_100k_fused"]["fused"], S=16, a=1, grid=391, counters=28)
    assert plans["k_w16_1m"]["paths"] == ["two_launch"]


def test_switch_values(plans):
    # order: LEVELWISE FUSED CLIMB SM3CLIMB PAIR SM3X NOSUB LATSCHED; tri-states: -1 automatic
    assert plans["k_w2_10k"]["switches"] == [0, -1, -1, 0, -1, -1, 0, 0]
    assert plans["parse_a"]["switches"] == [1, -1, 1, 1, 0, -1, 0, 1]
    assert plans["parse_b"]["switches"] == [0, -1, -1, 0, 1, 0, 1, 0]
