"""The coalescer's queue protocol and staging layout (csrc/coalesce_queue.h) without a GPU.

tests/cpp/coalesce_queue_test.cpp instantiates the protocol of coalesced_run with a CPU stand-in for run_batch and
is built twice, with -fsanitize=thread and with -fsanitize=address,undefined; each case below is one child process
(the BCOSGPU_COALESCE_* variables are read once per process), nothing is loaded into Python.

protocol: T threads x K calls of the three kinds mixed (n = 1 mostly, 2..7, now and then over kMaxBatch items;
strides 65 / 70, 128 / 64 / 200, 64 / 65; outputs set or null), the stand-in sleeping 20-220 us, throwing in ~1 %
of the batches and failing ~1 %.  The program itself checks every call's values, failed calls' untouched outputs,
the batches' kind, arrival order and size, the batches in flight against slots_in_use() and the cap past
BCOSGPU_COALESCE_DEEP callers, and the statistics; it exits 0 iff nothing was violated and 3 if a call never
returned.
boundary: one slot, a held batch and two arrivals behind it: kMaxBatch - 1 and 1 items are one batch, kMaxBatch and 1
are two, a job over kMaxBatch runs alone.
quiesce: one slot, two callers, round after round: the second call arrives just as the first one's batch ends and
nobody calls afterwards, so an arrival that neither the leader's drain nor q.idle accounts for stays stranded
(exit 3 after 10 s).
layout: stage_in / scatter_out single-threaded in staging buffers of exactly the staged sizes.
"""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SANITIZERS = {"tsan": ["-fsanitize=thread"],
              "asan": ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}
# (environment, threads, calls per thread)
CONFIGS = {
    "default-64": ({}, 64, 300),
    "default-256": ({}, 256, 100),
    "lockfree0": ({"BCOSGPU_COALESCE_LOCKFREE": "0"}, 64, 200),
    "slots1": ({"BCOSGPU_COALESCE_SLOTS": "1"}, 32, 200),
    "slots16-deep0": ({"BCOSGPU_COALESCE_SLOTS": "16", "BCOSGPU_COALESCE_DEEP": "0"}, 64, 200),
    "deep8": ({"BCOSGPU_COALESCE_DEEP": "8"}, 32, 200),  # reaches the cap without 128 threads
}


@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx is not None, "g++ not found"
    out = {}
    for name, flags in SANITIZERS.items():
        out[name] = str(tmp_path_factory.mktemp("coalesce_queue") / ("coalesce_queue_test_" + name))
        # (-Wextra but for the aggregate initialisation of SigJob, whose engine fields keep their defaults)
        subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Wno-missing-field-initializers", "-Werror"]
                       + flags + ["-o", out[name], os.path.join(ROOT, "tests", "cpp", "coalesce_queue_test.cpp"),
                                  "-lpthread"], check=True)
    return out


def _run(exe, args, env, timeout):
    full = {k: v for k, v in os.environ.items() if not k.startswith("BCOSGPU_COALESCE_")}
    full.update(env)
    r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=timeout, env=full)
    assert r.returncode == 0 and r.stderr == "", "exit %d\n%s\n%s" % (r.returncode, r.stdout[-4000:], r.stderr[-8000:])
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("config", list(CONFIGS))
@pytest.mark.parametrize("sanitizer", list(SANITIZERS))
def test_protocol(exes, sanitizer, config):
    env, threads, calls = CONFIGS[config]
    res = _run(exes[sanitizer], ["protocol", str(threads), str(calls)], env, timeout=180)
    print(res)
    assert res["nviolations"] == 0 and res["violations"] == []
    assert res["calls"] == threads * calls == res["ok_calls"] + res["failed_calls"] == res["stat_jobs"]
    assert res["stat_items"] == res["ok_items"] and res["ok_batches"] <= res["batches"]
    assert res["max_inflight"] <= res["slots"]
    # the run met what it is there for: failed batches, multi-item and over-kMaxBatch jobs
    assert res["failed_calls"] > 0 and res["big_jobs"] > 0 and res["items"] > res["calls"]
    if config == "default-64":
        # it really coalesced and overlapped: >= 10 % fewer batches than calls, >= 2 stand-in batches at once
        assert res["batches"] <= 0.9 * res["calls"] and res["max_inflight"] >= 2
        assert (res["slots"], res["deep"], res["lockfree"]) == (4, 128, 1)
    if config == "deep8":
        # batches were held to the cap of 2 in flight.  (default-256 passes DEEP too, but the program holds a batch
        # to the cap only when the callers it can be sure of -- the owners of its own and the running batches' jobs -- number DEEP,
        # and whether 128 of 256 do at some moment depends on the machine's load: it is printed, not asserted.)
        assert res["cap_checked"] > 0
    if config == "slots1":
        assert res["max_inflight"] == 1
    if config == "lockfree0":
        assert res["lockfree"] == 0


@pytest.mark.parametrize("sanitizer", list(SANITIZERS))
def test_batch_item_limit(exes, sanitizer):
    res = _run(exes[sanitizer], ["boundary"], {"BCOSGPU_COALESCE_SLOTS": "1"}, timeout=120)
    print(res)
    assert res["nviolations"] == 0
    assert res["cases"] == [[65535, 1, 1], [65536, 1, 2], [65537, 1, 2]]


@pytest.mark.parametrize("sanitizer,rounds", [("tsan", 20000), ("asan", 60000)])
def test_no_arrival_stranded_when_the_queue_goes_quiet(exes, sanitizer, rounds):
    res = _run(exes[sanitizer], ["quiesce", str(rounds)], {"BCOSGPU_COALESCE_SLOTS": "1"}, timeout=180)
    print(res)
    assert res["nviolations"] == 0 and res["rounds"] == rounds and rounds <= res["batches"] <= 2 * rounds


def test_layout(exes):
    res = _run(exes["asan"], ["layout"], {}, timeout=120)
    print(res)
    assert res["nviolations"] == 0 and res["batches"] >= 1000
