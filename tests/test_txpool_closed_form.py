"""The index-order rule of transaction admission in closed form against the literal restatement
(tests/txpool_restatement.py), on random batches dense in repeated nonces, repeated transactions and failing
checks.  No GPU, no signatures: a transaction here is its decoded fields, a hash that is a function of the
preimage fields, and a signature verdict.

Closed form: the independent verdict I(j) is steps 1-8 against the sets as they were before the call.  Group the
batch by nonce value; W is the lowest index of a group with I(W) = 0; every j > W of the group with I(j) not in
{2, 10004, 10007, 10006, 4} gets 10004 if hash(j) = hash(W), else 10000; everything else keeps I(j); the winners'
nonces and hashes enter the sets.
"""
import copy
import hashlib
import random

from txpool_restatement import (ALREADY_IN_TXPOOL, INVALID_CHAIN_ID, INVALID_GROUP_ID, MALFORMED, NONCE_CHECK_FAIL,
                                NONCE_FOR_HOST, OK, Pool, Tx)

OUT_OF_GROUP = {MALFORMED, ALREADY_IN_TXPOOL, INVALID_GROUP_ID, INVALID_CHAIN_ID, NONCE_FOR_HOST}


def make(rng):
    """A random transaction: few nonces, few recipients, every way to fail."""
    if rng.random() < 0.05:
        return Tx(None, bytes(32), bytes(20), False)
    f = {"group_id": b"group0" if rng.random() < 0.9 else b"other",
         "chain_id": b"chain0" if rng.random() < 0.9 else b"other",
         "nonce": rng.choice([b"", b"0", b"1", b"2", b"3", b"07", b"7", b"+1", str(2 ** 256 - 1).encode()]),
         "block_limit": rng.choice([100, 101, 105, 110, 111]), "to": rng.choice([b"a", b"b"])}
    h = hashlib.sha256(repr(sorted(f.items())).encode()).digest()  # equal hashes <=> equal preimages
    return Tx(f, h, b"\x01" * 20, rng.random() < 0.8)


def closed_form(pool, txs):
    """Statuses by the closed form; updates the pool's sets with the winners."""
    before = copy.deepcopy(pool)
    indep = [copy.deepcopy(before)._verify_and_submit(t) for t in txs]  # each against the untouched sets
    out = list(indep)
    groups = {}
    for j, t in enumerate(txs):
        if indep[j] not in OUT_OF_GROUP:
            groups.setdefault(t.nonce, []).append(j)
    for members in groups.values():
        accepted = [j for j in members if indep[j] == OK]
        if not accepted:
            continue
        w = accepted[0]
        for j in members:
            if j > w:
                out[j] = ALREADY_IN_TXPOOL if txs[j].hash == txs[w].hash else NONCE_CHECK_FAIL
        pool.nonces.add(txs[w].nonce)
        pool.hashes.add(txs[w].hash)
    return out


def test_closed_form_equals_the_literal_order():
    rng = random.Random(6)
    for trial in range(400):
        literal = Pool(0, b"chain0", b"group0", 10, 100)
        literal.ledger = {3}
        warm = [make(rng) for _ in range(rng.randint(0, 4))]
        for t in warm:
            literal._verify_and_submit(t)
        closed = copy.deepcopy(literal)
        txs = [make(rng) for _ in range(rng.randint(1, 24))]
        want = [literal._verify_and_submit(t) for t in txs]
        assert closed_form(closed, txs) == want, trial
        assert (closed.nonces, closed.hashes, closed.ledger) == (literal.nonces, literal.hashes, literal.ledger)
