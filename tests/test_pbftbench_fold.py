"""tools/pbftbench.py's baseline leg A' folds its row verdicts with whole-array numpy operations.  This checks
that fold, on the CPU, against a plain per-message loop over the same rows, for all-valid rows (what the
benchmark runs) and for seeded patterns of failed rows -- a wrong baseline would make the benchmark's
acceptance meaningless."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fisco-bcos_amd", "tools"))


def loop_fold(legs):
    ok = legs.ap_ok == 1
    flags = [0 if ok[r] else 2 for r in legs.msg_row]
    for i, r in legs.prop_row:
        flags[i] |= 0 if ok[r] else 4
    prep = []
    for i, r, cnt in legs.prep_seg:
        code = 1 if not ok[r:r + cnt].all() else 2 if int(legs.row_weight[r:r + cnt].sum()) < legs.quorum else 0
        prep.append(code)
        flags[i] |= 8 if code else 0
    own = list(flags)
    for parent, first, count in legs.groups:
        if any(own[first:first + count]):
            flags[parent] |= 16
        if int(legs.msg_weight[first:first + count].sum()) < legs.quorum:
            flags[parent] |= 32
    return flags, prep


def test_vectorised_fold_matches_loop(oracle):
    import pbftbench
    world = pbftbench.World(oracle, 0, seed=5)
    rng = np.random.default_rng(6)
    shapes = world.shapes()
    for shape, msgs, groups in shapes:
        legs = pbftbench.Legs(world, msgs, groups)
        patterns = [np.ones(legs.rows, dtype=np.uint8), np.zeros(legs.rows, dtype=np.uint8)]
        patterns += [(rng.random(legs.rows) > p).astype(np.uint8) for p in (0.002, 0.05, 0.5)]
        for k in range(min(legs.rows, 5)):  # one failed row at a time, at the start and the end
            for r in (k, legs.rows - 1 - k):
                one = np.ones(legs.rows, dtype=np.uint8)
                one[r] = 0
                patterns.append(one)
        for pat in patterns:
            legs.ap_ok = pat
            flags, prep = legs.fold()
            want_flags, want_prep = loop_fold(legs)
            assert flags.tolist() == want_flags, shape
            assert prep.tolist() == want_prep, shape
        legs.ap_ok = patterns[0]
        assert not legs.fold()[0].any(), shape
    # a group below the quorum: a NewView of 66 view changes
    shape, msgs, groups = shapes[2]
    legs = pbftbench.Legs(world, msgs[:67], [(0, 1, 66)])
    legs.ap_ok = np.ones(legs.rows, dtype=np.uint8)
    assert legs.fold()[0].tolist() == [32] + [0] * 66 == loop_fold(legs)[0]
