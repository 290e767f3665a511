"""Host-side mirror of the reference's prover interface for the state-transition AIR.

Names and argument meaning follow the reference so tests read like its own:
  ProofOptions(num_queries, blowup_factor, grinding_factor, hash_fn, field_extension, fri_folding_factor,
               fri_max_remainder)                          -- winterfell::ProofOptions as used at src/lib.rs:78-86
  TransactionMetadata                                      -- src/lib.rs:183-232 (field for field)
  TransactionProver(options).build_trace(tx_metadata)     -- src/prover.rs:20-98
  TransactionProver.get_pub_inputs(trace)                  -- src/prover.rs:106-129
  TransactionProver.commit_and_evaluate(...)               -- the hot half of Prover::prove (src/lib.rs:140):
        interpolate -> LDE -> Blake3 row hashes -> Merkle tree -> constraint evaluations
All device work goes through the C ABI (include/cstark.h); there is no CPU path here.
"""
import collections
import contextlib

import numpy as np

_P = 2**62 + 2**56 + 2**55 + 1  # the prime of f63::BaseElement
import torch

from . import _lib
from .backend import Backend, to_numpy_u64

TRACE_WIDTH = _lib.TX_TRACE_WIDTH
TRANSACTION_CYCLE_LENGTH = _lib.TX_CYCLE_LENGTH
PREV_TREE_ROOT_POS = 58  # src/merkle/constants.rs:45


class ProofOptions:
    """The 7 fields of winterfell::ProofOptions; defaults are the reference's (src/lib.rs:78-86)."""
    BLAKE3_256, SHA3_256 = 0, 1
    EXT_NONE, EXT_QUADRATIC, EXT_CUBIC = 0, 1, 2

    def __init__(self, num_queries=42, blowup_factor=8, grinding_factor=0, hash_fn=0, field_extension=0,
                 fri_folding_factor=4, fri_max_remainder=256):
        if blowup_factor & (blowup_factor - 1) or blowup_factor < 2:
            raise ValueError("blowup factor must be a power of two >= 2")
        self.num_queries, self.blowup_factor, self.grinding_factor = num_queries, blowup_factor, grinding_factor
        self.hash_fn, self.field_extension = hash_fn, field_extension
        self.fri_folding_factor, self.fri_max_remainder = fri_folding_factor, fri_max_remainder

    @property
    def log_blowup(self):
        return self.blowup_factor.bit_length() - 1


# cstark_witness_verdict by value: what Backend.tx_witness_check's verdict bytes mean
WITNESS_VERDICTS = ("VALID", "INDEX_RANGE", "SELF_TRANSFER", "SENDER_LEAF", "SENDER_PATH", "BALANCE", "MIDDLE_ROOT", "RECEIVER_LEAF", "NEXT_ROOT",
                    "SIGNATURE")


class WitnessCheck:
    """What a witness check found: ok; first_bad (the first transfer whose verdict is not VALID, None when ok) and verdict, the name of
    its verdict (WITNESS_VERDICTS; "VALID" when ok); n_bad; verdicts uint8 [n_tx]; final_root [7], the root the batch leaves as the
    device folded it, whatever the verdicts; folds [n_tx][4][7] when they were asked for."""

    def __init__(self, report, verdicts, folds=None):
        self.n_tx, self.depth, self.n_bad = int(report.n_tx), int(report.merkle_depth), int(report.n_bad)
        self.first_bad = None if report.first_bad < 0 else int(report.first_bad)
        self.verdict = WITNESS_VERDICTS[int(report.first_verdict)]
        self.verdicts, self.folds = verdicts, folds
        self.final_root = np.array(list(report.final_root), np.uint64)

    @property
    def ok(self):
        return self.first_bad is None

    def __str__(self):
        return "consistent" if self.ok else "transfer %d: %s (%d of %d transfers bad)" % (self.first_bad, self.verdict, self.n_bad, self.n_tx)

    def __repr__(self):
        return "WitnessCheck(%s)" % self


class TransactionMetadata:
    """Series of transfers in the account tree (src/lib.rs:183-194); arrays are uint64 in BaseElement memory form."""
    FIELDS = ("initial_roots", "final_root", "s_old_values", "r_old_values", "s_indices", "r_indices",
              "s_paths", "r_paths", "deltas", "sig_rx", "sig_s")

    def __init__(self, initial_roots, final_root, s_old_values, r_old_values, s_indices, r_indices, s_paths, r_paths,
                 deltas, sig_rx, sig_s):
        n = len(initial_roots)
        # "Enforce that all vectors are of equal length" (src/lib.rs:211-218)
        for name, a in (("s_old_values", s_old_values), ("r_old_values", r_old_values), ("s_indices", s_indices),
                        ("r_indices", r_indices), ("s_paths", s_paths), ("r_paths", r_paths), ("deltas", deltas),
                        ("sig_rx", sig_rx), ("sig_s", sig_s)):
            if len(a) != n:
                raise ValueError("%s has %d entries, expected %d" % (name, len(a), n))
        self.initial_roots = np.ascontiguousarray(initial_roots, np.uint64).reshape(n, 7)
        self.final_root = np.ascontiguousarray(final_root, np.uint64).reshape(7)
        self.s_old_values = np.ascontiguousarray(s_old_values, np.uint64).reshape(n, 14)
        self.r_old_values = np.ascontiguousarray(r_old_values, np.uint64).reshape(n, 14)
        self.s_indices = np.ascontiguousarray(s_indices, np.uint64).reshape(n)
        self.r_indices = np.ascontiguousarray(r_indices, np.uint64).reshape(n)
        self.s_paths = np.ascontiguousarray(s_paths, np.uint64)
        self.r_paths = np.ascontiguousarray(r_paths, np.uint64)
        self.deltas = np.ascontiguousarray(deltas, np.uint64).reshape(n)
        self.sig_rx = np.ascontiguousarray(sig_rx, np.uint64).reshape(n, 6)
        self.sig_s = np.ascontiguousarray(sig_s, np.uint8).reshape(n, 32)
        self.n_tx = n
        self.depth = self.s_paths.shape[1] - 1
        if self.s_paths.shape != (n, self.depth + 1, 7) or self.r_paths.shape != self.s_paths.shape:
            raise ValueError("authentication paths must be [n][depth+1][7]")
        if (self.depth + 1) & self.depth:
            raise ValueError("tree depth must be one less than a power of 2")  # src/lib.rs:102-105

    @classmethod
    def load(cls, path):
        z = np.load(path)
        return cls(*[z[f] for f in cls.FIELDS])

    @classmethod
    def build_random(cls, num_transactions, depth=15, seed=0x5EED):
        """Counterpart of TransactionMetadata::build_random (src/lib.rs:235-465), seeded: cstark_tx_witness_generate
        (host code of the library; no GPU involved)."""
        import ctypes as C
        n, d = int(num_transactions), int(depth)
        arrays = dict(initial_roots=np.zeros((n, 7), np.uint64), final_root=np.zeros(7, np.uint64),
                      s_old_values=np.zeros((n, 14), np.uint64), r_old_values=np.zeros((n, 14), np.uint64),
                      s_indices=np.zeros(n, np.uint64), r_indices=np.zeros(n, np.uint64),
                      s_paths=np.zeros((n, d + 1, 7), np.uint64), r_paths=np.zeros((n, d + 1, 7), np.uint64),
                      deltas=np.zeros(n, np.uint64), sig_rx=np.zeros((n, 6), np.uint64), sig_s=np.zeros((n, 32), np.uint8))
        s = _lib.TxWitnessStruct()
        s.n_tx, s.merkle_depth = n, d
        for f, a in arrays.items():
            setattr(s, f, a.ctypes.data_as(_lib.u8p if f == "sig_s" else _lib.u64p))
        _lib.check(_lib.load().cstark_tx_witness_generate(C.byref(s), C.c_uint64(seed)))
        return cls(*[arrays[f] for f in cls.FIELDS])

    def save(self, path):
        np.savez_compressed(path, **{f: getattr(self, f) for f in self.FIELDS})

    def check(self, backend=None, check_signatures=False, want_folds=False):
        """Is this witness consistent?  Every transfer's indices, leaves, paths, balance and roots (and, with check_signatures, its
        signature) tested on the GPU in one launch, before any trace is built -> WitnessCheck: .ok, .first_bad, .verdict
        ("SENDER_PATH", ...), .verdicts, .final_root.  n_tx need not be a power of two.  A witness resident in the backend is left
        alone (cstark_tx_witness_check)."""
        return WitnessCheck(*(backend or Backend()).tx_witness_check(self, check_signatures=check_signatures, want_folds=want_folds))


class TransferRefused(Exception):
    """Ledger.apply refused the batch at transfer `index`; nothing changed.  reason: one of Ledger.REASONS (cstark_ledger_reason)."""

    def __init__(self, index, reason):
        super().__init__("transfer %d refused: %s" % (index, Ledger.REASONS.get(reason, reason)))
        self.index, self.reason = index, reason


def check_account_paths(indices, paths, roots, values=None, present=None, backend=None, want_roots=False):
    """Authentication paths from anywhere (an AccountOpening, a witness's s_paths / r_paths, a file) against the roots they state, on
    the GPU: -> one cstark_path_verdict per path (0 = valid, Backend.PATH_*); see Backend.account_check_paths.  No ledger is needed."""
    return (backend or Backend()).account_check_paths(indices, paths, roots, values=values, present=present, want_roots=want_roots)


class AccountOpening:
    """What Ledger.open returns: the accounts at `indices` (values [count][14], present [count]) with their authentication paths
    ([count][depth + 1][7], the witness's path form; an absent account's leaf is the all-zero digest) under `root`."""

    def __init__(self, indices, values, present, paths, root, backend=None):
        self.indices, self.values, self.present, self.paths, self.root = indices, values, present, paths, root
        self._backend = backend

    @property
    def depth(self):
        return self.paths.shape[1] - 1

    def check(self, backend=None):
        """the verdict of every path against `root`, with the leaf test on (values, present): all zero for an honest opening"""
        return check_account_paths(self.indices, self.paths, self.root, self.values, self.present, backend=backend or self._backend)


MultiproofCheck = collections.namedtuple("MultiproofCheck", "verdict at root n_merges")


def check_account_multiproof(depth, indices, nodes, root, values=None, present=None, leaves=None, backend=None):
    """One Merkle multiproof from anywhere (an AccountMultiOpening, a file, a peer) against the root it states, on the GPU: ->
    MultiproofCheck(verdict, at, root, n_merges); verdict 0 = valid, Backend.MULTI_*; see Backend.account_check_multiproof.  indices are
    strictly ascending as given: an untrusted proof's order is data, and a wrong one is the verdict INDEX.  No ledger is needed."""
    return MultiproofCheck(*(backend or Backend()).account_check_multiproof(depth, indices, nodes, root, values=values, present=present, leaves=leaves))


UpdateCheck = collections.namedtuple("UpdateCheck", "verdict at new_root n_changed")


def check_account_update(depth, indices, old_values, new_values, nodes, old_root, new_root=None, old_present=None, new_present=None, backend=None):
    """A claimed change of state checked by someone who holds only roots, on the GPU: the multi-opening (indices, old_values,
    old_present, nodes) under old_root, and the same accounts' new values -> UpdateCheck(verdict, at, new_root, n_changed); verdict 0 =
    valid, Backend.UPDATE_*; see Backend.account_check_update.  new_root=None computes the root the change leads to.  Both states are
    folded in one pass that shares the proof nodes.  No ledger is needed."""
    return UpdateCheck(*(backend or Backend()).account_check_update(depth, indices, old_values, new_values, nodes, old_root, new_root=new_root,
                                                                    old_present=old_present, new_present=new_present))


class AccountMultiOpening:
    """What Ledger.open_multi returns: the accounts at the ascending, distinct `indices` (values [count][14], present [count]) and ONE
    multiproof for all of them under `root`: nodes [n_nodes][7], the siblings no opened leaf accounts for, level `depth` first and
    ascending within a level (include/cstark.h).  inverse[k] is the position in `indices` of the k-th index the caller asked for;
    nbytes is what travels: indices, values, presence flags, nodes and root."""

    def __init__(self, depth, indices, values, present, nodes, root, inverse, backend=None):
        self.depth, self.indices, self.values, self.present, self.nodes, self.root, self.inverse = depth, indices, values, present, nodes, root, inverse
        self._backend = backend

    @property
    def nbytes(self):
        return self.indices.nbytes + self.values.nbytes + self.present.size + self.nodes.nbytes + self.root.nbytes

    def check(self, backend=None):
        """-> MultiproofCheck: verdict 0 for an honest opening, .root the fold, .n_merges the merges it took"""
        return check_account_multiproof(self.depth, self.indices, self.nodes, self.root, self.values, self.present, backend=backend or self._backend)

    def to_ledger(self, backend=None):
        """-> Ledger.from_opening(self): a partial ledger that knows exactly these accounts"""
        return Ledger.from_opening(self, backend=backend)

    def check_update(self, new_values, new_present=None, new_root=None, backend=None):
        """-> UpdateCheck: this opening as the old state under .root, new_values [count][14] (new_present [count], None: all present)
        as the new state of the same accounts, in the order of .indices.  With new_root the transition .root -> new_root is checked;
        without it .new_root of the answer is the root the change leads to."""
        return check_account_update(self.depth, self.indices, self.values, new_values, self.nodes, self.root, new_root=new_root,
                                    old_present=self.present, new_present=new_present, backend=backend or self._backend)


class Ledger:
    """The account tree an operator holds, resident on the GPU (cstark_ledger_*): set_accounts, then apply(transfers) per batch -- the
    counterpart of the sequential loop of TransactionMetadata::build_random (src/lib.rs:341-422) on real accounts and transfers.
    apply() leaves the batch's witness resident in the backend: backend.prove(options) follows without an upload."""
    APPLIED, INDEX_RANGE, SELF_TRANSFER, ABSENT, BALANCE, SIGNATURE, UNKNOWN, KEY, HELD, NOT_REACHED = 0, 1, 2, 3, 4, 5, 6, 7, 8, 9
    REASONS = {1: "index out of range", 2: "sender equals receiver", 3: "account absent", 4: "delta above the sender's balance",
               5: "signature does not verify", 6: "account not among those a partial ledger knows",
               7: "secret is not the secret of the sender's public key",
               8: "an earlier candidate of the same sender was refused in this selection", 9: "enough candidates were selected before this one"}

    def __init__(self, depth=15, backend=None):
        self.backend = backend or Backend()
        self.depth = int(depth)
        self._led = self.backend.ledger_create(self.depth)

    @classmethod
    def from_opening(cls, opening, backend=None):
        """-> a PARTIAL ledger built from an AccountMultiOpening, or from (depth, indices, values, present, nodes, root), under the root
        the opening states (cstark_ledger_create_partial): it knows exactly the opened accounts, present or absent, and for them it
        behaves as the full ledger does -- apply (the witness stays resident for prove), set_accounts, root, open, open_multi,
        checkpoints, audit.  A transfer that names an unknown account is refused with reason UNKNOWN, every other call with an unknown
        index raises CstarkError.  One opening per ledger.  Raises ValueError carrying the verdict (.verdict, .at: Backend.MULTI_*) when
        the opening does not fold to its root or has no shape."""
        if isinstance(opening, AccountMultiOpening):
            backend = backend or opening._backend
            opening = (opening.depth, opening.indices, opening.values, opening.present, opening.nodes, opening.root)
        depth, indices, values, present, nodes, root = opening
        backend = backend or Backend()
        led, verdict, at = backend.ledger_create_partial(int(depth), indices, values, present, nodes, root)
        if led is None:
            err = ValueError("the opening gives no ledger: verdict %d (at %d)" % (verdict, at))
            err.verdict, err.at = verdict, at
            raise err
        self = cls.__new__(cls)
        self.backend, self.depth, self._led = backend, int(depth), led
        return self

    @property
    def partial(self):
        """True for a ledger built by from_opening"""
        return self.backend.ledger_partial_info(self._led)[0]

    def partial_info(self):
        """-> (is_partial, n_known, n_opaque): opened indices and proof nodes of a partial ledger; (False, accounts, 0) of a full one"""
        return self.backend.ledger_partial_info(self._led)

    def known(self, indices):
        """-> bool [count]: the leaves this ledger knows (a full ledger: every index below 2^depth)"""
        return self.backend.ledger_known(self._led, indices)

    def close(self):
        if getattr(self, "_led", None) and getattr(self.backend, "ctx", None):
            self.backend.ledger_destroy(self._led)
        self._led = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_accounts(self, indices, values):
        """bulk insert or overwrite: distinct leaf indices, values [count][14] (pk.x pk.y balance nonce, memory form)"""
        self.backend.ledger_set_accounts(self._led, indices, values)

    def root(self, at=None):
        """the current root, or with at=checkpoint the root at that checkpoint"""
        return self.backend.ledger_root(self._led) if at is None else self.backend.ledger_root_at(self._led, at)

    def accounts(self, indices):
        """-> (values [count][14], present [count])"""
        return self.backend.ledger_get_accounts(self._led, indices)

    def open(self, indices, at=None):
        """-> AccountOpening: values, presence and authentication paths of the given leaves under the current root (indices may repeat
        and may name absent accounts: that is a proof of absence).  Read-only.  at=checkpoint: the same as the ledger was at that
        checkpoint, under the root a proof of that moment binds (an account created since is absent)."""
        idx = np.ascontiguousarray(indices, np.uint64).reshape(-1)
        return AccountOpening(idx, *self.backend.ledger_open_accounts(self._led, self.depth, idx, at=at), backend=self.backend)

    def open_multi(self, indices, at=None):
        """-> AccountMultiOpening: the given leaves (in any order, repeats allowed: they are sorted and de-duplicated here, and
        .inverse maps the request back) with ONE multiproof for all of them instead of a path each: the siblings that paths under one
        root share travel once, and those an opened leaf accounts for not at all.  Absent accounts are proven absent.  Read-only: one
        gather on the GPU, no hashing.  at=checkpoint: under the root of that checkpoint, as open()."""
        asked = np.ascontiguousarray(indices, np.uint64).reshape(-1)
        idx, inverse = np.unique(asked, return_inverse=True)
        return AccountMultiOpening(self.depth, idx, *self.backend.ledger_open_multi(self._led, self.depth, idx, at=at), inverse=inverse.reshape(-1),
                                   backend=self.backend)

    def open_multi_for(self, transfers, at=None):
        """-> AccountMultiOpening of the distinct senders and receivers of `transfers` (what apply() takes): everything a batch reads,
        for someone who does not hold the tree: .to_ledger() gives them a partial ledger that applies the batch and leaves its witness
        resident for prove, and .check_update(*ledger.accounts(opening.indices), new_root=ledger.root()) confirms the transition."""
        if hasattr(transfers, "s_indices"):
            transfers = (transfers.s_indices, transfers.r_indices)
        named = np.concatenate([np.ascontiguousarray(transfers[0], np.uint64).reshape(-1), np.ascontiguousarray(transfers[1], np.uint64).reshape(-1)])
        return self.open_multi(named, at=at)

    def checkpoint(self):
        """-> an id that names the ledger's state as it is now (an integer >= 1, never reused).  No device work; old states are kept by
        not overwriting them, so apply() costs what it costs without one.  At most 16 are live at once (CstarkError -5 beyond)."""
        return self.backend.ledger_checkpoint(self._led)

    def revert(self, cp):
        """the ledger goes back to checkpoint cp: root, accounts and openings of that moment; checkpoints taken after cp are dropped,
        cp stays live.  The resident witness is left alone: it is still the last applied batch's."""
        self.backend.ledger_revert(self._led, cp)

    def release(self, cp):
        """checkpoint cp ends; the current state and the other checkpoints are unchanged"""
        self.backend.ledger_release(self._led, cp)

    def audit(self, at=None):
        """-> the audit report of the current state (or of checkpoint `at`): .consistent, .n_bad, the first failing node as .first_kind
        (Backend.NODE_EMPTY / NODE_LEAF / NODE_INNER), .first_level, .first_index; .n_nodes; .slots_live / .slots_held / .slots_free of
        the whole ledger.  Every stored node is hashed from its stored children on the GPU, in one launch.  Read-only."""
        return self.backend.ledger_audit(self._led, 0 if at is None else at)

    def apply(self, transfers, want_witness=True, check_signatures=False):
        """transfers: (s_indices, r_indices, deltas, sig_rx, sig_s) or an object with these attributes (a TransactionMetadata, say).
        Applies them in order and returns the batch's TransactionMetadata (None with want_witness=False: the witness stays on the
        device only); raises TransferRefused, with ledger and resident witness unchanged, at the first transfer that cannot be applied.
        By default signatures are copied through, not checked -- and TransactionAir does not bind them either: a batch with a forged
        signature still proves and verifies.  check_signatures=True (cstark_ledger_apply_checked) checks every transfer's signature on
        the device first, against the message the transfer signs (sender's key, receiver's key, delta, the sender's nonce as the
        transfers before it leave it), and refuses the batch with reason SIGNATURE at the first bad one."""
        if hasattr(transfers, "s_indices"):
            transfers = tuple(getattr(transfers, f) for f in ("s_indices", "r_indices", "deltas", "sig_rx", "sig_s"))
        at, reason, arrays = self.backend.ledger_apply(self._led, self.depth, *transfers, want_witness=want_witness,
                                                       check_signatures=check_signatures)
        if at >= 0:
            raise TransferRefused(at, reason)
        return None if arrays is None else TransactionMetadata(*[arrays[f] for f in TransactionMetadata.FIELDS])

    @staticmethod
    def _unsigned(transfers):
        if hasattr(transfers, "s_indices"):
            return tuple(getattr(transfers, f) for f in ("s_indices", "r_indices", "deltas"))
        return tuple(transfers[:3])

    def messages(self, transfers):
        """-> uint64 [n][28]: the message each transfer of the batch has to sign (sender's key, receiver's key, delta, the sender's
        nonce as the transfers before it leave it, two zeros).  transfers: (s_indices, r_indices, deltas, ...) or an object with these
        attributes.  Raises TransferRefused where apply() would, with its reason.  Read-only."""
        at, reason, out = self.backend.ledger_messages(self._led, *self._unsigned(transfers))
        if at >= 0:
            raise TransferRefused(at, reason)
        return out

    def sign(self, transfers, secrets, seed=0, max_attempts=256):
        """-> (s_indices, r_indices, deltas, sig_rx, sig_s), exactly what apply() takes: the batch signed on the device with the senders'
        secret keys (secrets[t] signs transfer t).  Raises TransferRefused where apply() would, with its reason, or with reason KEY at
        the first transfer whose secret is not the secret of its sender's public key.  Read-only.  Secrets are small integers,
        1 .. 255 (public_keys): a signer for building batches, tests and benchmarks.  It is not a wallet."""
        s, r, d = (np.ascontiguousarray(a, np.uint64).reshape(-1) for a in self._unsigned(transfers))
        at, reason, rx, ss, _ = self.backend.ledger_sign(self._led, s, r, d, secrets, seed=seed, max_attempts=max_attempts)
        if at >= 0:
            raise TransferRefused(at, reason)
        return s, r, d, rx, ss

    def select(self, transfers, want, check_signatures=True, pow2=True, apply=False, chunk=0, want_messages=False):
        """-> Selection: a provable batch out of a pool of candidate transfers in arrival order (cstark_ledger_select).  transfers:
        (s_indices, r_indices, deltas, sig_rx, sig_s) or an object with these attributes; the signatures may be left out (or None)
        without check_signatures and apply.  Nothing is refused as a whole: every candidate gets a status -- APPLIED (0, selected), a
        reason of apply(), HELD (an earlier candidate of the same sender was refused in this call: the sender is held for the rest of
        it, though the account still receives) or NOT_REACHED (`want` were selected before it).  Candidates are examined in order against
        the accounts as the selected ones before them leave them; check_signatures checks the signatures on the device in passes of
        `chunk` candidates (0: the library's choice), whatever the bad candidates do.  pow2: the selection is cut to the largest power
        of two it holds, what prove() needs.  apply: the selection is applied as apply(selection.transfers) would apply it and its
        witness is resident for prove(); otherwise the call is read-only."""
        if hasattr(transfers, "s_indices"):
            transfers = tuple(getattr(transfers, f, None) for f in ("s_indices", "r_indices", "deltas", "sig_rx", "sig_s"))
        s, r, d = (np.ascontiguousarray(a, np.uint64).reshape(-1) for a in transfers[:3])
        rx, ss = (tuple(transfers[3:5]) + (None, None))[:2]
        B = self.backend
        flags = (B.SELECT_CHECK_SIGNATURES if check_signatures else 0) | (B.SELECT_POW2 if pow2 else 0) | (B.SELECT_APPLY if apply else 0)
        status, selected, messages, report, arrays = B.ledger_select(self._led, self.depth, s, r, d, rx, ss, want, flags=flags, chunk=chunk,
                                                                     want_messages=want_messages)
        witness = None if arrays is None else TransactionMetadata(*[arrays[f] for f in TransactionMetadata.FIELDS])
        pool = (s, r, d, None if rx is None else np.ascontiguousarray(rx, np.uint64).reshape(-1, 6),
                None if ss is None else np.ascontiguousarray(ss, np.uint8).reshape(-1, 32))
        return Selection(status, selected, pool, report, messages, witness)


class Selection:
    """What Ledger.select returns.  status: uint8 [n], one cstark_ledger_reason per candidate (Ledger.APPLIED = 0: selected);
    selected: the selected candidate numbers, ascending; transfers: the five arrays of the selection, what Ledger.apply takes (the
    signatures None when the pool had none); counts: candidates per status, a list of ten; report: n_candidates, n_selected,
    n_sig_checked, n_chunks, root_after; messages: [n][28] with want_messages (the message of every candidate sent to the device, zeros
    elsewhere); witness: the TransactionMetadata of the applied selection (apply=True and something selected), else None."""

    def __init__(self, status, selected, pool, report, messages=None, witness=None):
        self.status, self.selected, self.report, self.messages, self.witness = status, selected, report, messages, witness
        self.transfers = tuple(None if a is None else a[selected] for a in pool)
        self.counts = [int(k) for k in report.counts]

    def __len__(self):
        return len(self.selected)


def public_keys(secrets, backend=None):
    """-> uint64 [count][12]: secrets[i] * G, the public key (x, y in memory form) of each secret in 1 .. 255, computed on the device:
    words 0..11 of an account of Ledger.set_accounts."""
    return (backend or Backend()).schnorr_public_keys(secrets)


class TransactionProver:
    """MI355X counterpart of src/prover.rs::TransactionProver plus the hot half of Prover::prove."""

    def __init__(self, options=None, backend=None):
        self.options = options or ProofOptions()
        self.backend = backend or Backend()
        self._bufs = {}

    def _buf(self, name, shape, dtype=torch.int64):
        t = self._bufs.get(name)
        if t is None or tuple(t.shape) != tuple(shape) or t.dtype != dtype:
            t = torch.empty(shape, dtype=dtype, device=self.backend.device)
            self._bufs[name] = t
        return t

    # -- src/prover.rs:37-98
    def load_witness(self, tx_metadata):
        self.backend.upload_witness(tx_metadata)
        self.n_tx, self.depth = tx_metadata.n_tx, tx_metadata.depth
        self.trace_length = self.n_tx * TRANSACTION_CYCLE_LENGTH
        if self.trace_length & (self.trace_length - 1):
            raise ValueError("the number of transactions must be a power of two")

    def build_trace(self, tx_metadata=None):
        if tx_metadata is not None:
            self.load_witness(tx_metadata)
        return self.backend.build_trace(self._buf("trace", (TRACE_WIDTH, self.trace_length)))

    # -- src/prover.rs:106-129
    @staticmethod
    def get_pub_inputs(trace):
        first = to_numpy_u64(trace[PREV_TREE_ROOT_POS:PREV_TREE_ROOT_POS + 7, 0])
        last = to_numpy_u64(trace[PREV_TREE_ROOT_POS:PREV_TREE_ROOT_POS + 7, -1])
        return first, last  # initial_root, final_root

    # -- hot half of Prover::prove
    def extend_and_commit(self, trace, k0=0, nk=None):
        """interpolate -> LDE (cosets [k0,k0+nk)) -> leaf hashes; returns (coeffs, lde, nodes)."""
        b, lb = self.backend, self.options.log_blowup
        n = trace.shape[1]
        nk = (1 << lb) - k0 if nk is None else nk
        coeffs = b.interpolate_columns(trace, out=self._buf("coeffs", (TRACE_WIDTH, n)))
        lde = b.lde_columns(coeffs, lb, k0=k0, nk=nk, out=self._buf("lde", (nk, TRACE_WIDTH, n)))
        L = n << lb
        nodes = self._buf("nodes", (2 * L, 32), torch.uint8)
        b.hash_rows(lde, lb, k0=k0, leaves=nodes[L:])
        return coeffs, lde, nodes

    def build_tree(self, nodes):
        return self.backend.merkle_build(nodes)

    def evaluate_constraints(self, lde, coeffs_struct, pub_inputs4, k0=0, input_is_lde=False):
        """input_is_lde: `lde` is this prover's own extension of the whole trace (all cosets): degree-split evaluation, same values."""
        n = lde.shape[2]
        return self.backend.evaluate_constraints(lde, coeffs_struct, pub_inputs4, self.depth, self.options.log_blowup, k0=k0,
                                                 out=self._buf("combined", (lde.shape[0], n)), input_is_lde=input_is_lde)

    # -- Prover::prove as called at src/lib.rs:140 (trace generation included: the trace never leaves HBM)
    def prove(self, tx_metadata=None):
        """Full proof of the loaded transactions -> serialised proof bytes (layout: include/cstark.h)."""
        if tx_metadata is not None:
            self.load_witness(tx_metadata)
        return self.backend.prove(self.options)


@contextlib.contextmanager
def _proof_form(backend, compact):
    """prove(compact=True): the backend's proof form set to "compact" (one Merkle multiproof per tree, include/cstark.h) for one prove()
    and restored after it.  compact=False leaves the backend as it is: the proof takes Backend.proof_form, "plain" unless set."""
    if not compact:
        yield
        return
    before = backend.proof_form
    backend.proof_form = "compact"
    try:
        yield
    finally:
        backend.proof_form = before


def get_example_options():
    """The options of get_example (src/lib.rs:75-89)."""
    return ProofOptions(42, 8, 0, ProofOptions.BLAKE3_256, ProofOptions.EXT_NONE, 4, 256)


class TransactionExample:
    """src/lib.rs:92-150 without the random witness synthesis: holds options + metadata, proves and verifies on the GPU.
    verify() checks a proof against this example's public inputs (first initial root, final root) with cstark_tx_verify and
    raises VerifierError on rejection, as the reference's verify returns Err(VerifierError)."""

    def __init__(self, options, tx_metadata, backend=None):
        self.options, self.tx_metadata = options, tx_metadata
        self.prover = TransactionProver(options, backend)

    def prove(self, compact=False):
        with _proof_form(self.prover.backend, compact):
            return self.prover.prove(self.tx_metadata)

    def verify(self, proof):
        """winterfell::verify::<TransactionAir>(proof, pub_inputs) (src/lib.rs:144-150): the proof's own options are accepted."""
        from .verify import VerifierError
        initial_root, final_root = self.pub_inputs()
        v = int(self.prover.backend.tx_verify([proof], initial_root, final_root)[0])
        if v != 0:
            raise VerifierError(v)

    def convert(self, proof, compact=True):
        """the verified proof in the compact form (compact=False: the plain form), the bytes prove(compact=...) writes; raises
        VerifierError when verify() would (cstark_tx_convert)"""
        initial_root, final_root = self.pub_inputs()
        return _converted_or_raise(*self.prover.backend.tx_convert([proof], initial_root, final_root, _form_name(compact)))

    def pub_inputs(self):
        return self.tx_metadata.initial_roots[0], self.tx_metadata.final_root

    def check_witness(self, check_signatures=False, want_folds=False):
        """TransactionMetadata.check of this example's witness on its own backend -> WitnessCheck; str() of it names the first
        inconsistent transfer and what is wrong with it, e.g. "transfer 3: SENDER_PATH (1 of 8 transfers bad)".  Unlike validate() it
        builds no trace and, with check_signatures, it catches a forged signature, which still proves and verifies."""
        return self.tx_metadata.check(self.prover.backend, check_signatures=check_signatures, want_folds=want_folds)

    def validate(self, want_cycles=False, want_frame=False):
        """Trace::validate of the reference's debug builds, on the device: builds the trace of this example's witness and checks every
        transition constraint and the statement verify() would be given (cstark_air_validate_trace).  -> TraceReport; str(report) names
        the first violation, e.g. "transfer 3, row 126, constraint 99"."""
        trace = self.prover.build_trace(self.tx_metadata)
        return self.prover.backend.air_validate_trace(Backend.AIR_TRANSACTION, trace, self.tx_metadata.depth, np.concatenate(self.pub_inputs()),
                                                      want_cycles=want_cycles, want_frame=want_frame)


# ---- the standalone examples of the reference: same prove() surface over cstark_air_prove ---------------------------------------
def _air_verify_or_raise(backend, proof, air, public_inputs=None, numbers=None):
    """winterfell::verify::<Air>(proof, pub_inputs) through cstark_air_verify: the proof's own options are accepted"""
    from .verify import VerifierError
    v = int(backend.air_verify([proof], air, public_inputs, numbers=numbers)[0])
    if v != 0:
        raise VerifierError(v)


def _form_name(compact):
    return "compact" if compact else "plain"


def _converted_or_raise(converted, verdicts):
    from .verify import VerifierError
    if int(verdicts[0]) != 0:
        raise VerifierError(int(verdicts[0]))
    return converted[0]


def _air_convert_or_raise(backend, proof, compact, air, public_inputs=None, numbers=None):
    """_air_verify_or_raise that returns the proof in the other form (cstark_air_convert)"""
    return _converted_or_raise(*backend.air_convert([proof], air, public_inputs, _form_name(compact), numbers=numbers))


class _ResidentWitness:
    """An example's witness is uploaded by its first prove() and stays in device memory (any other upload on the same backend replaces
    it).  While it is resident the host arrays it was uploaded from are READ-ONLY (numpy refuses writes), so a changed witness can never
    be proved from the stale device copy: call invalidate() before editing them (or assign new arrays: that is detected)."""

    def _witness_arrays(self):
        raise NotImplementedError

    def _ensure_resident(self, upload):
        arrays = self._witness_arrays()
        key = tuple(id(a) for a in arrays)
        if getattr(self.backend, "resident", None) is not self or getattr(self, "_resident_key", None) != key:
            upload()
            self.backend.resident, self._resident_key = self, key
            self._was_writeable = [bool(a.flags.writeable) for a in arrays]
            for a in arrays:
                a.flags.writeable = False

    def invalidate(self):
        """the host witness is about to change: make it writable again and upload it anew at the next prove()"""
        if getattr(self, "_resident_key", None) is not None:
            for a, w in zip(self._witness_arrays(), self._was_writeable):
                if w:
                    a.flags.writeable = True
        self._resident_key = None
        if getattr(self.backend, "resident", None) is self:
            self.backend.resident = None


class MerkleExample(_ResidentWitness):
    """merkle::update::MerkleExample (src/merkle/update/mod.rs:36-127): proves the Merkle-update half of the transfers with the
    65-register MerkleAir."""

    def __init__(self, options, tx_metadata, backend=None):
        self.options, self.tx_metadata = options, tx_metadata
        self.backend = backend or Backend()

    def _witness_arrays(self):
        return [getattr(self.tx_metadata, f) for f in TransactionMetadata.FIELDS]

    def prove(self, compact=False):
        """The witness is uploaded by the first call and stays resident (_ResidentWitness: read-only on the host until invalidate())."""
        self._ensure_resident(lambda: self.backend.upload_witness(self.tx_metadata))
        with _proof_form(self.backend, compact):
            return self.backend.air_prove(Backend.AIR_MERKLE, self.options)

    def pub_inputs(self):
        return self.tx_metadata.initial_roots[0], self.tx_metadata.final_root

    def verify(self, proof):
        """src/merkle/update/mod.rs:109-127; raises VerifierError on rejection, like TransactionExample.verify"""
        _air_verify_or_raise(self.backend, proof, Backend.AIR_MERKLE, np.concatenate(self.pub_inputs()))

    def convert(self, proof, compact=True):
        """as TransactionExample.convert"""
        return _air_convert_or_raise(self.backend, proof, compact, Backend.AIR_MERKLE, np.concatenate(self.pub_inputs()))

    def validate(self, want_cycles=False, want_frame=False):
        """as TransactionExample.validate, for the MerkleAir trace of the witness"""
        self._ensure_resident(lambda: self.backend.upload_witness(self.tx_metadata))
        return self.backend.air_validate_trace(Backend.AIR_MERKLE, self.backend.merkle_build_trace(), self.tx_metadata.depth,
                                               np.concatenate(self.pub_inputs()), want_cycles=want_cycles, want_frame=want_frame)


class SchnorrExample(_ResidentWitness):
    """schnorr::SchnorrExample (src/schnorr/mod.rs:52-186): messages [n][28] (public key || 16 elements) with signatures."""

    def __init__(self, options, messages, sig_rx, sig_s, backend=None):
        self.options, self.messages, self.sig_rx, self.sig_s = options, messages, sig_rx, sig_s
        self.backend = backend or Backend()

    @classmethod
    def build_random(cls, options, num_signatures, seed=0x5EED, backend=None):
        import ctypes as C
        n = int(num_signatures)
        msg, rx, s = np.zeros((n, 28), np.uint64), np.zeros((n, 6), np.uint64), np.zeros((n, 32), np.uint8)
        _lib.check(_lib.load().cstark_schnorr_witness_generate(C.c_uint32(n), C.c_uint64(seed), msg.ctypes.data_as(_lib.u64p),
                                                               rx.ctypes.data_as(_lib.u64p), s.ctypes.data_as(_lib.u8p)))
        return cls(options, msg, rx, s, backend)

    @classmethod
    def sign(cls, secrets, payloads, seed=0, options=None, backend=None, max_attempts=256):
        """An example over chosen signers and payloads: message i = public key of secrets[i] || payloads[i] (16 words in memory form),
        as src/schnorr/mod.rs:94-99, keys and signatures made on the device (Backend.schnorr_public_keys, schnorr_sign).  Secrets are
        small integers, 1 .. 255: a signer for building batches, tests and benchmarks.  It is not a wallet.  Raises ValueError when a
        signature found no accepted attempt among max_attempts."""
        backend = backend or Backend()
        sk = np.ascontiguousarray(secrets, np.uint64).reshape(-1)
        messages = np.zeros((sk.size, 28), np.uint64)
        messages[:, 12:] = np.ascontiguousarray(payloads, np.uint64).reshape(sk.size, 16)
        messages[:, :12] = backend.schnorr_public_keys(sk)
        rx, s, _, status = backend.schnorr_sign(messages, sk, seed=seed, max_attempts=max_attempts)
        if status.any():
            raise ValueError("signature %d found no accepted attempt among %d" % (int(np.flatnonzero(status)[0]), max_attempts))
        return cls(options or get_example_options(), messages, rx, s, backend)

    def _witness_arrays(self):
        return [self.messages, self.sig_rx, self.sig_s]

    def prove(self, compact=False):
        """The witness is uploaded by the first call and stays resident (_ResidentWitness: read-only on the host until invalidate())."""
        self._ensure_resident(lambda: self.backend.upload_schnorr_witness(self.messages, self.sig_rx, self.sig_s))
        with _proof_form(self.backend, compact):
            return self.backend.air_prove(Backend.AIR_SCHNORR, self.options)

    def check(self):
        """verify_signature (src/schnorr/mod.rs:220-245) for every signature of this example, on the device: verdicts uint8 [n]
        (Backend.SIG_*: 0 = valid).  Runs beside a resident witness without touching it."""
        return self.backend.schnorr_check(self.messages, self.sig_rx, self.sig_s)

    def verify(self, proof):
        """src/schnorr/mod.rs:175-186 through cstark_schnorr_verify: the statement is every message and signature of this example; the
        proof's own options are accepted.  Raises VerifierError on rejection"""
        from .verify import VerifierError
        v = int(self.backend.schnorr_verify([proof], [self])[0])
        if v != 0:
            raise VerifierError(v)

    def convert(self, proof, compact=True):
        """as TransactionExample.convert, through cstark_schnorr_convert"""
        return _converted_or_raise(*self.backend.schnorr_convert([proof], [self], _form_name(compact)))

    def validate(self, want_cycles=False, want_frame=False):
        """as TransactionExample.validate: the SchnorrAir trace against the resident statement; a forged signature shows as a failing
        boundary entry at the last row of its block (str(report): "boundary entry 55: register 0 at step 1023")"""
        self._ensure_resident(lambda: self.backend.upload_schnorr_witness(self.messages, self.sig_rx, self.sig_s))
        return self.backend.air_validate_trace(Backend.AIR_SCHNORR, self.backend.schnorr_build_trace(), 0, True,
                                               want_cycles=want_cycles, want_frame=want_frame)


class RescueExample:
    """RescueExample of benches/rescue.rs:25-102: a chain of `chain_length` Rescue hashes from the bench's seed 42..48 (held in memory
    form, R = 2^64).  The public inputs -- seed and result -- are read from the trace inside the prover, as get_pub_inputs does."""

    def __init__(self, chain_length, options, backend=None, seed=None):
        if chain_length & (chain_length - 1) or chain_length < 8:
            raise ValueError("chain length must a power of 2")   # benches/rescue.rs:34-37 (at least 8 links: 64 trace rows)
        self.options, self.chain_length = options, int(chain_length)
        self.backend = backend or Backend()
        r2 = pow(2, 64, _P)
        self.seed = np.array([(v * r2) % _P for v in range(42, 49)], np.uint64) if seed is None else np.ascontiguousarray(seed, np.uint64)

    def prove(self, compact=False):
        with _proof_form(self.backend, compact):
            return self.backend.rescue_prove(self.options, self.seed, self.chain_length)

    def pub_inputs(self):
        """seed and result; the result is the rate half of the chain's last row (RescueProver::get_pub_inputs, benches/rescue.rs:331-354),
        read from a trace built on the device the first time it is asked for"""
        if getattr(self, "_result", None) is None:
            trace = self.backend.rescue_chain_build_trace(self.seed, self.chain_length)
            self._result = to_numpy_u64(trace[:7, -1])
        return self.seed, self._result

    def verify(self, proof):
        """benches/rescue.rs:88-94; raises VerifierError on rejection"""
        _air_verify_or_raise(self.backend, proof, Backend.AIR_RESCUE_CHAIN, np.concatenate(self.pub_inputs()))

    def convert(self, proof, compact=True):
        """as TransactionExample.convert"""
        return _air_convert_or_raise(self.backend, proof, compact, Backend.AIR_RESCUE_CHAIN, np.concatenate(self.pub_inputs()))

    def validate(self, want_cycles=False, want_frame=False):
        """as TransactionExample.validate: the chain's trace against seed and result"""
        trace = self.backend.rescue_chain_build_trace(self.seed, self.chain_length)
        return self.backend.air_validate_trace(Backend.AIR_RESCUE_CHAIN, trace, 0, np.concatenate(self.pub_inputs()),
                                               want_cycles=want_cycles, want_frame=want_frame)


class RangeProofExample:
    """range::RangeProofExample (src/range/mod.rs:28-110): `number` is a field element in memory form whose canonical value is
    below 2^63 (larger inputs are refused, src/range/tests.rs:54-62)."""

    def __init__(self, options, number, backend=None):
        self.options, self.number = options, int(number)
        self.backend = backend or Backend()

    def prove(self, compact=False):
        with _proof_form(self.backend, compact):
            return self.backend.air_prove(Backend.AIR_RANGE, self.options, self.number)

    def verify(self, proof):
        """src/range/mod.rs:103-110; raises VerifierError on rejection"""
        _air_verify_or_raise(self.backend, proof, Backend.AIR_RANGE, numbers=self.number)

    def convert(self, proof, compact=True):
        """as TransactionExample.convert"""
        return _air_convert_or_raise(self.backend, proof, compact, Backend.AIR_RANGE, numbers=self.number)

    def validate(self, want_cycles=False, want_frame=False):
        """as TransactionExample.validate: the 64-row accumulator trace against the number"""
        return self.backend.air_validate_trace(Backend.AIR_RANGE, self.backend.range_build_trace(self.number), 0, [self.number],
                                               want_cycles=want_cycles, want_frame=want_frame)
