"""One long-lived cstark_ctx driven through the catalogue of context_history_cases.py in many orders: every answer is compared with its
CPU expectation the moment it arrives, so a table found under the wrong key, a block that did not grow, a staging block rewritten too
early or a witness disturbed by a call that promised to leave it alone shows as the first operation whose answer differs, together with
the calls that came before it.  No GPU result is compared with another GPU result here, except inside the report of a mismatch (the
same operation once more on a fresh context: wrong alone, or only after that history)."""
import os
import subprocess
import sys

import pytest

import context_history_cases as H

pytestmark = pytest.mark.gpu
ROOT = H.ROOT


def fresh():
    from certificate_stark_amd.backend import Backend
    return H.Env(Backend())


def release(*envs):
    """closes the contexts of a test -- unless an operation ended in an unexpected error: a context that may have faulted is abandoned, not
    destroyed (no hipFree, no stream destruction), since nothing more is started on the GPU after a fault"""
    for env in envs:
        if STOPPED:
            env.backend.ctx = None
        else:
            env.backend.close()


def run_alone(op):
    """the mismatch report's extra run: the operation as the first call of a fresh context"""
    env = fresh()
    try:
        return H.first_difference(op, op.run(env), op.expectation)
    except Exception as e:
        STOPPED.append("%s raised %s on the fresh context of a mismatch report" % (op.name, type(e).__name__))
        raise
    finally:
        release(env)


STOPPED = []      # why nothing more is started: an operation ended in an error nobody expected, which may have been a fault of the GPU


def run_one(env, op, done, label):
    """one operation on env, checked at once; done: the names that ran on this context before it"""
    from certificate_stark_amd._lib import CstarkError
    if STOPPED:
        pytest.fail("not run: %s" % STOPPED[0])
    want = op.expectation                     # from the CPU side, before the GPU is asked
    history = "%s: after %d calls %s" % (label, len(done), done)
    if op.refused:
        try:
            op.run(env)
        except CstarkError as e:
            if e.code in (-1, -5):            # CSTARK_ERR_INVALID_ARG, CSTARK_ERR_UNSUPPORTED: a refusal
                return
            STOPPED.append("%s ended in status %d earlier in this module (%s)" % (op.name, e.code, label))
            raise AssertionError("%s\n%s was to be refused, but failed: %s" % (history, op.name, e)) from e
        pytest.fail("%s\n%s was not refused" % (history, op.name))
    try:
        got = op.run(env)
    except Exception as e:                    # a status the library returned (or a fault): nothing more is started
        STOPPED.append("%s raised %s earlier in this module (%s)" % (op.name, type(e).__name__, label))
        raise AssertionError("%s\n%s raised %s: %s" % (history, op.name, type(e).__name__, e)) from e
    diff = H.first_difference(op, got, want)
    if diff is not None:
        alone = run_alone(op)
        pytest.fail("%s\nfirst diverging operation: %s (after %s)\n%s\non a fresh context the same operation is %s" %
                    (history, op.name, done[-1] if done else "nothing: the first call", diff,
                     "RIGHT: wrong only after this history" if alone is None else "WRONG too (%s)" % alone))


def run_schedule(env, names, label):
    done = []
    for name in names:
        run_one(env, H.BY_NAME[name], done, label)
        done.append(name)


def on_one_context(names, label):
    env = fresh()
    try:
        run_schedule(env, names, label)
    finally:
        release(env)


# ---- a. near-collision pairs: A, B, A, B on one context, and from the other end ---------------------------------------------------------------
@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("name", sorted(H.PAIRS))
def test_near_collisions_answer_for_themselves(name, order):
    on_one_context(H.pair_schedules(name)[order], "pair %s, order %d" % (name, order))


# ---- b. ladders: smallest request, largest, smallest again, another block's owner in between ----------------------------------------------
@pytest.mark.parametrize("block", sorted(H.LADDERS))
def test_grow_only_blocks_up_down_up(block):
    on_one_context(H.ladder_schedule(block), "ladder of %s" % block)


# ---- c. shuffles ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", H.SHUFFLE_SEEDS)
def test_the_whole_catalogue_in_a_shuffled_order_twice(seed):
    order = H.shuffle_schedule(seed)
    print("seed %d:" % seed, order[:len(H.OPS)])
    on_one_context(order, "shuffle with seed %d" % seed)


# ---- d. a refused call changes nothing ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("refused", [op.name for op in H.REFUSED])
def test_a_refused_call_changes_nothing(refused):
    triples = [s for s in H.refusal_schedules() if s[1] == refused]
    assert len(triples) == 3
    on_one_context([name for s in triples for name in s], "G, X, G around %s" % refused)


# ---- e. two contexts in one thread -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("close_half_way", [False, True])
def test_two_contexts_alternating_call_by_call(close_half_way):
    a, b = H.two_context_schedules()
    first, second = fresh(), fresh()
    done_a, done_b = [], []
    try:
        for k, (x, y) in enumerate(zip(a, b)):
            run_one(first, H.BY_NAME[x], done_a, "first of two contexts (the second has run %s)" % done_b)
            done_a.append(x)
            if close_half_way and k == len(a) // 2:
                release(second)
            if not close_half_way or k < len(a) // 2:
                run_one(second, H.BY_NAME[y], done_b, "second of two contexts (the first has run %s)" % done_a)
                done_b.append(y)
    finally:
        release(first, second)


# ---- f. cold starts ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", H.FAMILIES)
def test_every_operation_as_the_first_call_of_a_context(family):
    names = [n for n in H.first_call_names() if H.BY_NAME[n].family == family]
    assert names
    for name in names:
        on_one_context([name], "cold start")


COLD_CONTEXTS = 8      # a condition on coverage, not a measured figure


def test_the_first_proof_of_eight_fresh_contexts():
    """the first call of a context builds every table it needs and uses it at once, with the trace forked onto the side streams"""
    for k in range(COLD_CONTEXTS):
        on_one_context(["tx_1_d3"], "fresh context %d of %d" % (k + 1, COLD_CONTEXTS))


CHILD = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
         "import context_history_cases as H\n"
         "from certificate_stark_amd.backend import Backend\n"
         "env = H.Env(Backend())\n"
         "print(H.proof_digest(H.BY_NAME['tx_1_d3'].run(env)))\n"
         "env.backend.close()\n") % (ROOT, os.path.join(ROOT, "tests"))


def test_the_first_proof_of_a_fresh_process_on_both_split_paths():
    """CSTARK_SPLIT_MERGE is read once per process: one fresh child per setting, each printing the SHA-256 of the first proof of its
    first context; both must be the CPU prover's"""
    want = H.proof_digest(H.BY_NAME["tx_1_d3"].expectation)
    for setting in ("1", "0"):
        child = subprocess.run([sys.executable, "-c", CHILD], env=dict(os.environ, CSTARK_SPLIT_MERGE=setting), capture_output=True, text=True, timeout=600)
        assert child.returncode == 0, "CSTARK_SPLIT_MERGE=%s: %s" % (setting, child.stderr[-2000:])      # a child that died: no second child
        assert child.stdout.strip().splitlines()[-1] == want, "CSTARK_SPLIT_MERGE=%s wrote another first proof than the CPU prover" % setting
