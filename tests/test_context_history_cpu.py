"""The catalogue of context_history_cases.py checked without a GPU: STATE names exactly the data members of struct cstark_ctx, every
expectation can be computed from the CPU side and is deterministic, and the schedules the GPU tests run cover what they claim to cover."""
import os

import numpy as np
import pytest

import context_history_cases as H

CTX_H = os.path.join(H.ROOT, "certificate-stark_amd", "csrc", "ctx.h")


def equal(a, b):
    if isinstance(a, bytes) or isinstance(b, bytes):
        return a == b
    return len(a) == len(b) and all(x.shape == y.shape and x.dtype == y.dtype and np.array_equal(x, y) for x, y in zip(a, b))


# ---- context members ------------------------------------------------------------------------------------------------------------------
def test_state_names_every_member_of_the_context_and_no_other():
    members = H.ctx_members(open(CTX_H).read())
    assert len(members) == len(set(members)) and len(members) > 50, members
    assert "part_ev" in members and "side2" in members and "wit" in members and "schnorr_seed_key" in members   # arrays, lists, brace initialisers
    missing = [m for m in members if m not in H.STATE]
    gone = [m for m in H.STATE if m not in members]
    assert not missing, "members of cstark_ctx without a class in STATE (add one, and a history case that reaches it): %s" % missing
    assert not gone, "STATE names members that cstark_ctx no longer has: %s" % gone


def test_the_member_parser_sees_a_new_member():
    text = open(CTX_H).read().replace("    void *ws = nullptr;", "    void *ws = nullptr;\n    uint64_t *dummy_block = nullptr, *dummy2[4] = {};")
    members = H.ctx_members(text)
    assert "dummy_block" in members and "dummy2" in members


def test_every_state_entry_is_classified_and_names_operations_that_touch_it():
    for member, s in H.STATE.items():
        assert s["cls"] in H.CLASSES, member
        if s["cls"] == "cache":
            assert s["key"], "a keyed cache states the fields its lookup compares: %s" % member
        if s["of"] is not None:
            assert s["of"] in H.STATE, member
        ops = H.ops_of(s["ops"])
        if s["cls"] not in ("handle", "timing"):
            assert ops, "no operation reaches %s" % member
        if s["ops"] != ["*"]:
            for op in ops:
                assert member in op.touches, "%s is said to touch %s but does not list it" % (op.name, member)
    for op in H.OPS:
        assert op.touches <= set(H.STATE), (op.name, op.touches - set(H.STATE))


def test_the_cache_keys_are_the_fields_the_lookups_compare():
    """the key fields of STATE against the text of the lookups: a field dropped from a comparison, or added to one, shows here"""
    capi = open(os.path.join(H.ROOT, "certificate-stark_amd", "csrc", "capi.hip")).read()
    prove = open(os.path.join(H.ROOT, "certificate-stark_amd", "csrc", "prove.hip")).read()
    import re
    patterns = {
        "plans": (r"for \(const NttPlan &p : c->plans\)\s*if \((.*?)\) \{", capi),
        "cosets": (r"for \(const CosetTable &t : c->cosets\)\s*if \((.*?)\) \{", capi),
        "steps": (r"for \(const cs::StepTable &t : c->steps\)\s*if \((.*?)\) \{", capi),
        "periodic": (r"for \(const PeriodicTable &t : c->periodic\)\s*if \((.*?)\) \{", capi),
        "small_periodic": (r"for \(const PeriodicTable &t : c->small_periodic\)\s*if \((.*?)\) \{", capi),
        "assert_inv": (r"for \(const cs::AssertInverseTable &t : c->assert_inv\)\s*if \((.*?)\) p\.agrp_inv", capi),
        "air_static": (r"for \(const cs::AirCombineStatic &q : c->air_static\)\s*if \((.*?)\) \{", capi),
        "raw_periodic": (r"for \(const cs::RawPeriodic &t : c->raw_periodic\)\s*if \((.*?)\) \{", capi),
        "arena": (r"if \(c->arena && (.*?)\) \{ \*out = c->arena;", prove),
    }
    lookups = {}
    for member, (pattern, text) in patterns.items():
        found = re.search(pattern, text, re.S)
        assert found, "the lookup of the cache `%s` is no longer written as this test reads it (pattern %r): restate the pattern" % (member, pattern)
        lookups[member] = found.group(1)
    for member, cond in lookups.items():
        compared = re.findall(r"(?:\b[pqt]\.|c->arena->)([\w.()]+?)\s*(?:==|>=)", cond)
        assert tuple(compared) == H.STATE[member]["key"], (member, compared)
    assert "memcmp(key, c->schnorr_seed_key, sizeof key)" in prove


# ---- expectations ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", H.FAMILIES)
def test_expectations_are_computable_deterministic_and_not_empty(family):
    for op in [op for op in H.OPS if op.family == family]:
        first = op.expectation
        assert first is op.expectation, "the expectation is memoised"
        for cached in (H.cpu_tx_proof, H.cpu_air_proof, H._ledger_model_applied, H.validate_case):      # the second evaluation starts from nothing
            cached.cache_clear()
        again = H.normalise(op._expect())
        assert equal(first, again), "%s: two evaluations of the expectation differ" % op.name
        if isinstance(first, bytes):
            assert len(first) > 0, op.name
        else:
            assert len(first) > 0 and all(isinstance(a, np.ndarray) for a in first) and sum(a.size for a in first) > 0, op.name
        if op.proof is not None:
            from tools.make_proof_digest import section_digests
            assert isinstance(first, bytes) and len(section_digests(first, *op.proof)) == 12, op.name


def test_expectations_tell_the_near_collisions_apart():
    """two operations of a near-collision set with one expectation would let a wrong cache hit pass"""
    for name, ops in H.PAIRS.items():
        if name == "resident_witness":
            continue
        seen = [H.BY_NAME[o].expectation for o in ops]
        for i in range(len(seen)):
            for j in range(i):
                assert not equal(seen[i], seen[j]), (name, ops[i], ops[j])


def test_the_catalogue_holds_what_the_history_tests_are_about():
    names = set(H.BY_NAME)
    assert {H.tx_name(n, d) for n, d in H.TX_SHAPES} <= names
    assert {H.tx_name(2, 3, k) for k in H.TX_OPTION_SETS} <= names
    assert len(H.REFUSED) == 7 and len(H.SHUFFLE_SEEDS) == 6
    assert [H.log_n_of(n) for n in H.LOG_N_10] == [10, 10, 10, 10]            # read from the expectations: four AIRs at one trace length
    assert {"transform", "commit", "tx_prove", "sub_air", "verify", "validate", "sig", "ledger", "refused"} == set(H.FAMILIES)
    # the verdict cases hold an accepted and a rejected proof
    for op in ("tx_verify", "air_verify", "schnorr_verify"):
        v = H.BY_NAME[op].expectation[0]
        assert v.any() and not v.all(), op
    # every altered trace has a violation to report, every clean one none
    for op in H.OPS:
        if op.family == "validate":
            assert (op.expectation[0][0] >= 0) == op.name.endswith("_cell"), op.name
    assert list(H.BY_NAME["sig_check_forged"].expectation[0]) == [0, 1]


# ---- schedules ------------------------------------------------------------------------------------------------------------------------
def test_schedules_are_pure_functions_of_their_seeds():
    a, b = H.all_schedules(), H.all_schedules()
    assert a == b
    assert all(name in H.BY_NAME for s in a.values() for name in s)
    for seed in H.SHUFFLE_SEEDS:
        s = H.shuffle_schedule(seed)
        assert sorted(s[:len(H.OPS)]) == sorted(H.BY_NAME) and s[:len(H.OPS)] == s[len(H.OPS):]
    assert len({tuple(H.shuffle_schedule(seed)) for seed in H.SHUFFLE_SEEDS}) == len(H.SHUFFLE_SEEDS)


def test_every_operation_runs_first_and_after_every_other_family():
    schedules = H.all_schedules()
    first = {s[0] for s in schedules.values()}
    assert not set(H.BY_NAME) - first, "never a context's first call: %s" % sorted(set(H.BY_NAME) - first)
    after = {name: set() for name in H.BY_NAME}
    for s in schedules.values():
        seen = set()
        for name in s:
            after[name] |= seen
            seen.add(H.BY_NAME[name].family)
    for name, fams in after.items():
        missing = set(H.FAMILIES) - fams - {H.BY_NAME[name].family}
        assert not missing, "%s never runs after %s" % (name, sorted(missing))


def test_every_near_collision_occurs_in_both_orders():
    schedules = H.all_schedules()
    for name, ops in H.PAIRS.items():
        follows = set()
        for k in range(2):
            s = schedules["pair:%s:%d" % (name, k)]
            follows |= set(zip(s, s[1:]))
        for a in ops:            # every member directly behind every other one
            for b in ops:
                assert a == b or (a, b) in follows, "%s: %s never runs directly behind %s" % (name, b, a)


def test_every_grow_only_block_has_a_ladder():
    blocks = {m for m, s in H.STATE.items() if s["cls"] == "block"}
    assert not blocks - set(H.LADDERS), "grow-only blocks without a ladder: %s" % sorted(blocks - set(H.LADDERS))
    for block, (small, large, other) in H.LADDERS.items():
        assert block in blocks
        assert block in H.BY_NAME[small].touches and block in H.BY_NAME[large].touches and small != large, block
        assert block not in H.BY_NAME[other].touches, block
        assert H.ladder_schedule(block) == [small, other, large, other, small]


def test_refusal_and_two_context_schedules():
    r = H.refusal_schedules()
    assert len(r) == 3 * len(H.REFUSED)
    for g, x, g2 in r:
        assert g == g2 and H.BY_NAME[x].refused and not H.BY_NAME[g].refused and H.BY_NAME[g].family != "refused"
    for x in H.REFUSED:
        assert len({H.BY_NAME[s[0]].family for s in r if s[1] == x.name}) == 3
    a, b = H.two_context_schedules()
    assert len(a) == len(b) >= 8
    assert all(H.log_n_of(x) != H.log_n_of(y) for x, y in zip(a, b))
