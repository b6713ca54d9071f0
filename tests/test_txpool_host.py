"""The host-testable groundwork of transaction admission with the pool's state (no GPU): the
canonical-nonce parser (csrc/nonce_parse.h), the growth policy of a key set (csrc/keyset_policy.h) and the probe
arithmetic (csrc/keyset.h).

tests/cpp/txpool_host_test.cpp drives the three headers; it is built once with -fsanitize=address,undefined and
run on its own (no Python in the process).  Every expected value below is derived by hand from the rules the
headers state: rehash when bound + incoming > capacity / 2, into the smallest power of two >= 4 (live + incoming)
and >= 8; the bound grows by n per insert batch, never shrinks on erase, and becomes the live count at a rehash.
"""
import json
import os
import random
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx is not None, "g++ not found"
    out = str(tmp_path_factory.mktemp("txpool_host") / "txpool_host_test")
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-o", out, os.path.join(ROOT, "tests", "cpp", "txpool_host_test.cpp")],
                   check=True)
    return out


def _parse(exe, strings):
    text = "".join((s.hex() or "-") + "\n" for s in strings)
    r = subprocess.run([exe, "parse"], input=text, check=True, capture_output=True, text=True)
    lines = r.stdout.splitlines()
    assert len(lines) == len(strings) and r.stderr == ""
    return [None if ln == "0" else int(ln.split()[1], 16) for ln in lines]


def test_parser_corners(exe):
    rejected = [b"00", b"01", b"+1", b"-1", b" 1", b"0x1", b"n1", b"1 ", b"1\x00", b"\xb1", b"/", b":",
                str(2 ** 256).encode(), b"9" * 78, b"1" + b"0" * 78, b"0" * 78, str(2 ** 256 + 10 ** 40).encode()]
    accepted = [b"", b"0", b"1", b"9", b"10", b"999999999", b"1000000000", b"4294967296", str(2 ** 64).encode(),
                str(2 ** 255).encode(), str(2 ** 256 - 1).encode(), str(10 ** 77).encode()]
    got = _parse(exe, rejected + accepted)
    assert got[:len(rejected)] == [None] * len(rejected)
    assert got[len(rejected):] == [int(s) if s else 0 for s in accepted]  # Python's int() is the reference here


def test_parser_random_canonical(exe):
    rng = random.Random(20260)
    values = [rng.getrandbits(rng.randint(1, 256)) for _ in range(2000)]
    assert _parse(exe, [str(v).encode() for v in values]) == values


def _policy(exe, *scripts):
    r = subprocess.run([exe, "policy"] + list(scripts), check=True, capture_output=True, text=True)
    assert r.stderr == ""
    return [json.loads(line) for line in r.stdout.splitlines()]


def test_policy_capacity_is_a_power_of_two_at_least_8(exe):
    news = [run[0] for run in _policy(exe, "0:", "1:", "8:", "9:", "1000:", "65536:")]
    assert [s["cap"] for s in news] == [8, 8, 8, 16, 1024, 65536]
    assert all(s["bound"] == 0 for s in news)


def test_policy_threshold_is_exactly_half(exe):
    (run,) = _policy(exe, "8:I4/0;I1/4")
    _, a, b = run
    assert a == {"op": "insert", "must": False, "cap": 8, "bound": 4, "rehashes": 0}  # 0 + 4 = half: no read
    assert b == {"op": "insert", "must": True, "cap": 32, "bound": 5, "rehashes": 1}  # 4 (4 + 1) = 20 -> 32
    (run,) = _policy(exe, "8:I5/0")  # one batch over half of an empty set: 4 (0 + 5) = 20 -> 32
    assert run[1] == {"op": "insert", "must": True, "cap": 32, "bound": 5, "rehashes": 1}


def test_policy_bound_does_not_shrink_on_erase_and_resets_at_a_rehash(exe):
    (run,) = _policy(exe, "8:I3/0;E3;I1/0;I1/1")
    _, a, e, b, c = run
    assert (a["bound"], e["bound"], e["cap"], e["rehashes"]) == (3, 3, 8, 0)
    assert b == {"op": "insert", "must": False, "cap": 8, "bound": 4, "rehashes": 0}  # 3 tombstones + 1 live
    # the true live count is 1: the rehash keeps capacity 8 (4 (1 + 1) = 8), drops the tombstones, bound = 1 + 1
    assert c == {"op": "insert", "must": True, "cap": 8, "bound": 2, "rehashes": 1}


def test_policy_capacity_chosen(exe):
    (run,) = _policy(exe, "8:C0/0;C1/0;C3/0;C1000/0;C3/5;C2/0;C8/120")
    assert [s["cap"] for s in run[1:]] == [8, 8, 16, 4096, 32, 8, 512]


def test_policy_three_five_hundred_and_twenty(exe):
    """3, 5 and 120 keys into capacity 8 are two rehashes, 8 -> 32 -> 512."""
    (run,) = _policy(exe, "8:I3/0;I5/3;I120/8")
    assert [(s["must"], s["cap"], s["bound"]) for s in run[1:]] == [(False, 8, 3), (True, 32, 8), (True, 512, 128)]
    # after every step the bound is at most half the capacity: a probe always meets an EMPTY slot
    assert all(2 * s["bound"] <= s["cap"] for s in run[1:])


@pytest.mark.parametrize("cap,h", [(8, 0), (8, 5), (8, 7), (64, 2 ** 64 - 1), (1024, 12345678901234567)])
def test_probe_walk_and_bound(exe, cap, h):
    r = subprocess.run([exe, "probe", str(cap), str(h)], check=True, capture_output=True, text=True)
    d = json.loads(r.stdout)
    first = h % cap
    assert d["once"] and d["first"] == first
    assert d["wraps"] == (0 if first == 0 else 1)  # the chain wraps past the table's end once
    assert d["err_before"] == 0 and d["err_last"] == 0
    assert d["last"] == (first + cap - 1) % cap  # the last EMPTY slot, not the tombstone at `first`
    assert d["tomb_kept"] and d["over"] == -1 and d["err_over"] == 1  # the bound sets the error bit, nothing spins
