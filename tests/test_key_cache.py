"""KeyCacheBook (csrc/key_cache.h): the registered-key cache's rules -- which key gets a table, when a sighted key
is promoted, what an id looks like -- pinned on the host.  A slip in one of them changes no verdict (it sends sealer
signatures to the generic kernels, or hands out the id of an unbuilt table), so no GPU parity test notices.  Every
expected value was derived by hand from the keyed_slots / poll_build / keyed_clear this header replaced.  No
device, no threads, no sleeps: tests/cpp/key_cache_test.cpp runs the scripted steps (its header lists them) and
prints JSON.  Capacity 8, promotion after 3 calls, unless a scenario says otherwise."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G1 = 1 << 16  # the id of index 0 under generation 1

L12 = "L+1,2"
REP6 = "5,5,5,5,5,5"
SCENARIOS = {
    "three_sightings": "8:3:C;%s;I;%s;%s;I;S;F1;%s;I" % (L12, L12, L12, L12),
    "once_per_call": "8:3:R9;L+%s;L+%s;L-%s;L-%s;L-%s;L-%s;I;L+%s" % ((REP6,) * 7),
    "build_in_flight": "8:3:L+1;L+1;L+1;S;%s;%s;%s;I;F1;L+2;I;L+2;L+2" % (L12, L12, L12),
    "sixteen_per_build": "64:3:L+1..20;L+1..20;L+1..20;I;S;L+1..20;F1;I;L+1..20;S;F1;L+1..20;I",
    "half_capacity": "8:3:L+1..6;L+1..6;L+1..6;I;S;F1;I;L+5,6;L+5,6;L+5,6;I;R11..14;I;R15;I;L+1,15;I",
    "full_arena": "8:3:R21..27;%s;%s;%s;S;F1;%s;I" % (L12, L12, L12, L12),
    "failed_build": "8:3:%s;%s;%s;S;F0;I;%s;S;F1;%s;I" % (L12, L12, L12, L12, L12),
    "build_not_started": "8:3:L+1;L+1;L+1;L+1;I",
    "registration": "8:3:L+1;L+1;I;R1,2,1;I;R1,2,1;I;Rx3;I;R3;I",
    "no_arena": "8:3:Rn1;I",
    "clear": "8:3:R1,2;L+3;L+3;L+3;S;I;C;I;F1;I;R1,2",
    "tags": "8:3:T0,5;T1,5;T32768,5;T32769,5;T32767,65535",
    "empty_short_cut": "8:3:L-1,2;I",
    "promotion_off": "8:0:L+1,2;I;R1;L+1,2;L+1,2;L+1,2;I",
    "sketch_reset": "8:3:L+1;L+1;L+1000..66535;I;L+1;I;L+1;L+1",
    "sketch_not_yet": "8:3:L+1;L+1;L+1000..66534;I;L+1",
}


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("g++ not found")
    exe = str(tmp_path_factory.mktemp("key_cache") / "key_cache_test")
    subprocess.run([cxx, "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-o", exe,
                    os.path.join(ROOT, "tests", "cpp", "key_cache_test.cpp")], check=True)
    r = subprocess.run([exe] + list(SCENARIOS.values()), check=True, capture_output=True, text=True)
    lines = r.stdout.splitlines()
    assert len(lines) == len(SCENARIOS)
    # the steps that answer something, in order
    return {name: [s for s in json.loads(line) if s["op"] not in ("started", "finished", "clear")]
            for name, line in zip(SCENARIOS, lines)}


def _sub(d, **want):
    got = {k: d[k] for k in want}
    assert got == want


def _pairs(keys, first):
    return [[k, first + i] for i, k in enumerate(keys)]


def test_third_sighting_starts_the_build(runs):
    a, i1, b, c, i3, d, i4 = runs["three_sightings"]
    for call in (a, b):
        _sub(call, all=False, ids=[-1, -1], build=[])
    _sub(i1, misses=2, seen=2, sightings=2, next=0)
    _sub(c, all=False, ids=[-1, -1], build=[[1, 0], [2, 1]])
    _sub(i3, keys=0, hits=0, misses=6, builds=0, promoted=0, next=2, pending=0)
    _sub(d, all=True, ids=[G1, G1 + 1], build=[])  # slot_id(gen 1, 0 / 1)
    _sub(i4, keys=2, hits=2, misses=6, builds=2, promoted=2, next=2, seen=0, gen=1)


def test_a_key_counts_once_per_call_and_only_in_named_calls(runs):
    reg, a, b, r1, r2, r3, r4, info, c = runs["once_per_call"]
    _sub(reg, all=True, ids=[0])
    for call in (a, b, r1, r2, r3, r4):  # six occurrences a call, two named calls, four unnamed: nothing yet
        _sub(call, all=False, ids=[-1] * 6, build=[])
    _sub(info, seen=1, sightings=2, hits=1, misses=36, next=1, builds=1)
    _sub(c, all=False, ids=[-1] * 6, build=[[5, 1]])  # the third named call


def test_build_in_flight_stops_counting(runs):
    a, b, c, d1, d2, d3, info, e, i2, f, g = runs["build_in_flight"]
    _sub(c, build=[[1, 0]])
    for call in (d1, d2, d3):  # key 1 pending, key 2 new: neither counted, nothing started
        _sub(call, all=False, ids=[-1, -1], build=[])
    _sub(info, pending=1, building=True, seen=1, sightings=3, misses=9, next=1, keys=0)
    _sub(e, all=False, ids=[-1], build=[])  # key 2's first sighting comes after the build
    _sub(i2, keys=1, promoted=1, builds=1, seen=1, sightings=1, pending=0, building=False)
    _sub(f, build=[])
    _sub(g, build=[[2, 1]])


def test_sixteen_keys_per_build(runs):
    a, b, c, i1, during, i2, d, e, i3 = runs["sixteen_per_build"]
    first, rest = list(range(1, 17)), list(range(17, 21))
    _sub(a, build=[])
    _sub(b, build=[])
    _sub(c, all=False, ids=[-1] * 20, build=_pairs(first, 0))
    _sub(i1, next=16, seen=20, sightings=16 * 3 + 4 * 2, misses=60)  # the other 4 were not counted in the third call
    _sub(during, all=False, build=[])
    _sub(i2, keys=16, promoted=16, builds=16, seen=4, sightings=8, misses=80)
    _sub(d, all=False, ids=list(range(16)) + [-1] * 4, build=_pairs(rest, 16))
    _sub(e, all=True, ids=list(range(20)), build=[])
    _sub(i3, keys=20, promoted=20, builds=20, next=20, hits=20, misses=100, seen=0)


def test_promotion_takes_half_the_capacity(runs):
    a, b, c, i1, i2, d1, d2, d3, i3, reg, i4, ninth, i5, e, i6 = runs["half_capacity"]
    _sub(c, ids=[-1] * 6, build=_pairs([1, 2, 3, 4], 0))
    _sub(i1, sightings=4 * 3 + 2 * 2, misses=18, next=4)
    _sub(i2, keys=4, promoted=4, builds=4, seen=2, sightings=4)
    for call in (d1, d2, d3):  # keys 5 and 6 are no longer counted: half of 8 is promoted
        _sub(call, all=False, ids=[-1, -1], build=[])
    _sub(i3, promoted=4, next=4, sightings=4, misses=24)
    _sub(reg, all=True, ids=[4, 5, 6, 7], build=_pairs([11, 12, 13, 14], 4), at=[0, 1, 2, 3])
    _sub(i4, keys=8, next=8, builds=8, registered=4, hits=4)
    _sub(ninth, all=False, ids=[-1], build=[], at=[])  # nothing to build: no build can fail, the call returns 0
    _sub(i5, keys=8, next=8, builds=8, misses=25)
    _sub(e, all=False, ids=[0, -1], build=[])
    _sub(i6, sightings=4, misses=27)


def test_full_arena_stops_promotion(runs):
    reg, a, b, c, d, info = runs["full_arena"]
    _sub(reg, all=True, ids=list(range(7)))
    _sub(c, build=[[1, 7]])  # key 2 reached its third sighting too, with no index left
    _sub(d, all=False, ids=[7, -1], build=[])
    _sub(info, keys=8, promoted=1, next=8, seen=1, sightings=4, hits=7, misses=8, builds=8)


def test_failed_build_consumes_its_indices(runs):
    a, b, c, i1, d, e, i2 = runs["failed_build"]
    _sub(c, build=[[1, 0], [2, 1]])
    _sub(i1, keys=0, pending=0, building=False, next=2, builds=0, promoted=0, seen=2, sightings=6)
    _sub(d, all=False, ids=[-1, -1], build=[[1, 2], [2, 3]])
    _sub(e, all=True, ids=[2, 3])
    _sub(i2, keys=2, builds=2, promoted=2, next=4)
    a, b, c, d, info = runs["build_not_started"]  # the launch failed: build_started never called
    _sub(c, build=[[1, 0]])
    _sub(d, all=False, ids=[-1], build=[[1, 1]])
    _sub(info, next=2, pending=0, building=False, keys=0, misses=4)


def test_registration(runs):
    a, b, i0, reg, i1, again, i2, plan, i3, retry, i4 = runs["registration"]
    _sub(i0, seen=1, sightings=2, misses=2)
    _sub(reg, all=True, ids=[0, 1, 0], build=[[1, 0], [2, 1]], at=[0, 1, 2])
    _sub(i1, keys=2, builds=2, registered=2, promoted=0, next=2, hits=3, misses=2, seen=0)
    _sub(again, all=True, ids=[0, 1, 0], build=[], at=[])
    _sub(i2, keys=2, builds=2, registered=2, next=2, hits=6)
    _sub(plan, ids=[-1], build=[[3, 2]], at=[0])  # its build fails: nothing published or counted
    _sub(i3, keys=2, builds=2, registered=2, next=3, hits=6, misses=2)
    _sub(retry, all=True, ids=[3], build=[[3, 3]])
    _sub(i4, keys=3, builds=3, registered=3, next=4, hits=7)
    reg, info = runs["no_arena"]
    _sub(reg, all=False, ids=[-1], build=[])
    _sub(info, keys=0, next=0, misses=1)


def test_clear(runs):
    reg, a, b, c, i1, i2, i3, again = runs["clear"]
    _sub(reg, ids=[0, 1])
    _sub(c, build=[[3, 2]])
    _sub(i1, keys=2, pending=1, building=True, next=3, gen=0, registered=2)
    want = dict(keys=0, pending=0, building=False, next=0, promoted=0, registered=0, gen=1, seen=0, hits=2, misses=3,
                builds=2)
    _sub(i2, **want)
    _sub(i3, **want)  # the build that was in flight publishes nothing
    _sub(again, all=True, ids=[G1, G1 + 1], build=[[1, 0], [2, 1]])


def test_generation_tag_is_15_bits(runs):
    ids = [s["id"] for s in runs["tags"]]
    assert ids == [5, G1 + 5, 5, G1 + 5, 0x7FFFFFFF]


def test_empty_cache_short_cut(runs):
    a, info = runs["empty_short_cut"]
    _sub(a, all=False, ids=[-7, -7], build=[])  # the ids are not written
    _sub(info, hits=0, misses=0, seen=0)
    a, info, reg, b, c, d, i2 = runs["promotion_off"]  # BCOSGPU_KEY_PROMOTE=0: a named call is a plain lookup
    _sub(a, all=False, ids=[-7, -7], build=[])
    _sub(info, hits=0, misses=0, seen=0)
    for call in (b, c, d):
        _sub(call, all=False, ids=[0, -1], build=[])
    _sub(i2, seen=0, misses=6, hits=1)


def test_sightings_sketch_is_bounded(runs):
    a, b, big, i1, c, i2, d, e = runs["sketch_reset"]
    _sub(big, all=False, build=[])
    _sub(i1, seen=65537, sightings=2 + 65536, misses=2 + 65536)
    _sub(c, build=[])  # key 1 had two sightings; the sketch was dropped, this is its first again
    _sub(i2, seen=1, sightings=1)
    _sub(d, build=[])
    _sub(e, build=[[1, 0]])
    a, b, big, i1, c = runs["sketch_not_yet"]  # 65,536 keys in the sketch: kept
    _sub(i1, seen=65536)
    _sub(c, build=[[1, 0]])
