"""Device plumbing for the C ABI: torch owns HBM allocations and the HIP stream, the library does the work.

Field-element buffers are torch.int64 tensors holding the uint64 bit patterns (BaseElement memory form).
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from ._lib import check, u64p, u8p


def _np_u64(a):
    return np.ascontiguousarray(a, dtype=np.uint64)


def to_numpy_u64(t):
    return t.detach().cpu().contiguous().numpy().view(np.uint64)


class ProofBatch:
    """The proofs of one batched call: a sequence of bytes objects, materialised on access."""

    def __init__(self, buf, stride, lens):
        self._buf, self._stride, self._lens = buf, stride, lens

    def __len__(self):
        return len(self._lens)

    def __getitem__(self, i):
        if isinstance(i, slice):
            return [self[k] for k in range(*i.indices(len(self)))]
        if i < 0:
            i += len(self)
        if not 0 <= i < len(self):
            raise IndexError(i)
        return self._buf[i * self._stride:i * self._stride + int(self._lens[i])].tobytes()

    def __iter__(self):
        return (self[i] for i in range(len(self)))

    def __eq__(self, other):
        return list(self) == list(other)


class TraceReport:
    """What cstark_air_validate_trace found: the first violated transition constraint (step = cycle * cycle length + row_in_cycle; None
    when every frame is clean), the number of cycles with a violated frame, and the first failing boundary entry (None: none, or not
    checked).  cycle_codes / frame_values are numpy arrays when they were asked for (frame_values only with a violation)."""

    def __init__(self, air, n, rep, cycle_codes=None, frame_values=None):
        self.air = air
        _, nc, cyc = _lib.air_trace_shape(air, n.bit_length() - 1)
        self.unit = _lib.AIR_CYCLE_NAMES[air]
        self.step = None if rep.step < 0 else int(rep.step)
        self.constraint = None if self.step is None else int(rep.constraint)
        self.cycle = None if self.step is None else self.step // cyc
        self.row_in_cycle = None if self.step is None else self.step % cyc
        self.bad_cycles = int(rep.bad_cycles)
        self.boundary = None if rep.boundary < 0 else int(rep.boundary)
        self.boundary_register = None if self.boundary is None else int(rep.boundary_register)
        self.boundary_step = None if self.boundary is None else int(rep.boundary_step)
        self.cycle_codes = cycle_codes
        self.frame_values = frame_values if self.step is not None else None

    @property
    def ok(self):
        return self.step is None and self.boundary is None

    def __str__(self):
        parts = []
        if self.step is not None:
            parts.append("%s %d, row %d, constraint %d" % (self.unit, self.cycle, self.row_in_cycle, self.constraint))
        if self.boundary is not None:
            parts.append("boundary entry %d: register %d at step %d" % (self.boundary, self.boundary_register, self.boundary_step))
        return "; ".join(parts) if parts else "clean"

    def __repr__(self):
        return "TraceReport(%s)" % self


class _Conversion:
    """The output arguments of one cstark_*_convert call: one buffer per proof, sized by cstark_proof_convert_bound (a proof whose
    layout does not parse has no bound and is never converted: its buffer is a single byte)"""

    def __init__(self, backend, form):
        if form not in backend.PROOF_FORMS:
            raise ValueError("form is 'plain' or 'compact', not %r" % (form,))
        self.form, self.bufs = backend.PROOF_FORMS.index(form), []

    def allocate(self, proofs):
        from .verify import convert_bound
        for p in proofs:
            try:
                cap = convert_bound(p, self.form)
            except ValueError:
                cap = 1
            self.bufs.append((C.c_uint8 * cap)())

    def args(self, count):
        out = (C.POINTER(C.c_uint8) * max(1, count))()
        caps = (C.c_size_t * max(1, count))()
        self.lens = (C.c_size_t * max(1, count))()
        for i, b in enumerate(self.bufs):
            out[i], caps[i] = C.cast(b, C.POINTER(C.c_uint8)), len(b)
        return (C.c_uint32(self.form), out, caps, self.lens)

    def results(self, verdicts):
        return [bytes(memoryview(b)[:self.lens[i]]) if int(verdicts[i]) == 0 else None for i, b in enumerate(self.bufs)]


class Backend:
    """One cstark_ctx bound to a torch device and the current torch stream."""

    def __init__(self, device=None):
        self.lib = _lib.load()
        if not torch.cuda.is_available():
            raise _lib.CstarkError(-2, "no HIP device visible (torch.cuda.is_available() is False); no CPU fallback")
        self.device = torch.device("cuda", torch.cuda.current_device() if device is None else device)
        torch.cuda.set_device(self.device)
        self.stream = torch.cuda.current_stream(self.device)
        ctx = C.c_void_p()
        check(self.lib.cstark_ctx_create(C.c_int(self.device.index), C.c_void_p(self.stream.cuda_stream), C.byref(ctx)))
        self.ctx = ctx
        self.n_tx = 0
        self.depth = 0
        self.resident = None   # the example object whose witness is in device memory (prover.MerkleExample / SchnorrExample), if any

    def close(self):
        if getattr(self, "ctx", None):
            self.lib.cstark_ctx_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def synchronize(self):
        check(self.lib.cstark_ctx_synchronize(self.ctx))

    def empty_u64(self, *shape):
        return torch.empty(shape, dtype=torch.int64, device=self.device)

    def from_numpy_u64(self, a):
        return torch.from_numpy(_np_u64(a).view(np.int64)).to(self.device)

    @staticmethod
    def _ptr(t, typ=u64p):
        assert t.is_contiguous()
        return C.cast(C.c_void_p(t.data_ptr()), typ)

    # ---- K1 ----
    @staticmethod
    def _witness_struct(w):
        """-> (TxWitnessStruct over w's arrays, the arrays it points into: keep them alive for the call)"""
        s = _lib.TxWitnessStruct()
        s.n_tx, s.merkle_depth = int(w.n_tx), int(w.depth)
        keep = []
        for f, typ in (("initial_roots", u64p), ("final_root", u64p), ("s_old_values", u64p), ("r_old_values", u64p),
                       ("s_indices", u64p), ("r_indices", u64p), ("s_paths", u64p), ("r_paths", u64p),
                       ("deltas", u64p), ("sig_rx", u64p), ("sig_s", u8p)):
            a = np.ascontiguousarray(getattr(w, f), dtype=np.uint8 if typ is u8p else np.uint64)
            keep.append(a)
            setattr(s, f, a.ctypes.data_as(typ))
        return s, keep

    def upload_witness(self, w):
        """w: any object with the TransactionMetadata arrays as numpy attributes (see prover.TransactionMetadata)."""
        self.resident = None
        s, keep = self._witness_struct(w)
        check(self.lib.cstark_tx_witness_upload(self.ctx, C.byref(s)))
        self.n_tx, self.depth = int(w.n_tx), int(w.depth)

    def build_trace(self, out=None):
        n = self.n_tx * _lib.TX_CYCLE_LENGTH
        if out is None:
            out = self.empty_u64(_lib.TX_TRACE_WIDTH, n)
        assert out.shape == (_lib.TX_TRACE_WIDTH, n) and out.dtype == torch.int64
        check(self.lib.cstark_tx_build_trace(self.ctx, self._ptr(out)))
        return out

    # ---- account ledger (cstark_ledger_*): the witness from accounts and transfers ----
    def ledger_create(self, depth):
        led = C.c_void_p()
        check(self.lib.cstark_ledger_create(self.ctx, C.c_uint32(depth), C.byref(led)))
        return led

    def ledger_create_partial(self, depth, indices, values, present, nodes, root):
        """cstark_ledger_create_partial: a ledger built from a multi-opening under `root` -> (handle or None, verdict, at); verdict:
        Backend.MULTI_* (0 = valid, the only one with a handle).  indices strictly ascending, values [count][14], present [count] or
        None (all present), nodes [n_nodes][7] or None.  The resident witness is not touched."""
        idx = _np_u64(indices).reshape(-1)
        val = _np_u64(values).reshape(-1, 14)
        if val.shape[0] != idx.size:
            raise ValueError("one 14-element value per index")
        pres = None if present is None else np.ascontiguousarray(present, np.uint8).reshape(-1)
        if pres is not None and pres.size != idx.size:
            raise ValueError("one present flag per index")
        nd = None if nodes is None else _np_u64(nodes).reshape(-1, 7)
        if nd is not None and nd.shape[0] == 0:
            nd = None
        r = _np_u64(root).reshape(7)
        led, verdict, at = C.c_void_p(), C.c_uint32(0), C.c_uint32(0)
        check(self.lib.cstark_ledger_create_partial(self.ctx, C.c_uint32(depth), C.c_uint32(idx.size), self._hptr(idx), self._hptr(val),
                                                    None if pres is None else self._hptr(pres, u8p), None if nd is None else self._hptr(nd),
                                                    C.c_uint32(0 if nd is None else nd.shape[0]), self._hptr(r), C.byref(led), C.byref(verdict),
                                                    C.byref(at)))
        return (led if led.value else None), verdict.value, at.value

    def ledger_known(self, led, indices):
        """cstark_ledger_known -> bool [count]: which leaves the ledger knows (a full ledger: every index below 2^depth)"""
        idx = _np_u64(indices).reshape(-1)
        out = np.zeros(idx.size, np.uint8)
        check(self.lib.cstark_ledger_known(self.ctx, led, C.c_uint32(idx.size), self._hptr(idx), self._hptr(out, u8p)))
        return out.astype(bool)

    def ledger_partial_info(self, led):
        """cstark_ledger_partial_info -> (is_partial, n_known, n_opaque)"""
        partial, n_known, n_opaque = C.c_uint32(0), C.c_uint64(0), C.c_uint64(0)
        check(self.lib.cstark_ledger_partial_info(self.ctx, led, C.byref(partial), C.byref(n_known), C.byref(n_opaque)))
        return bool(partial.value), n_known.value, n_opaque.value

    def ledger_destroy(self, led):
        self.lib.cstark_ledger_destroy(led)

    def ledger_set_accounts(self, led, indices, values):
        idx = _np_u64(indices).reshape(-1)
        val = _np_u64(values).reshape(-1, 14)
        if val.shape[0] != idx.size:
            raise ValueError("one 14-element value per index")
        check(self.lib.cstark_ledger_set_accounts(self.ctx, led, C.c_uint32(idx.size), self._hptr(idx), self._hptr(val)))

    def ledger_get_accounts(self, led, indices):
        """-> (values uint64 [count][14], present bool [count])"""
        idx = _np_u64(indices).reshape(-1)
        val, present = np.zeros((idx.size, 14), np.uint64), np.zeros(idx.size, np.uint8)
        check(self.lib.cstark_ledger_get_accounts(self.ctx, led, C.c_uint32(idx.size), self._hptr(idx), self._hptr(val), self._hptr(present, u8p)))
        return val, present.astype(bool)

    def ledger_root(self, led):
        root = np.zeros(7, np.uint64)
        check(self.lib.cstark_ledger_root(self.ctx, led, self._hptr(root)))
        return root

    def ledger_open_accounts(self, led, depth, indices, at=None):
        """cstark_ledger_open_accounts: -> (values [count][14], present bool [count], paths [count][depth + 1][7], root [7]): the
        accounts as ledger_get_accounts gives them and their authentication paths under the current root, in the witness's path form
        (absent accounts: an all-zero leaf).  Read-only: the ledger and the resident witness are as before.
        at: a checkpoint id -- cstark_ledger_open_accounts_at, the same under the root of that checkpoint."""
        idx = _np_u64(indices).reshape(-1)
        n = idx.size
        val, present = np.zeros((n, 14), np.uint64), np.zeros(n, np.uint8)
        paths, root = np.zeros((n, depth + 1, 7), np.uint64), np.zeros(7, np.uint64)
        out = (C.c_uint32(n), self._hptr(idx), self._hptr(val), self._hptr(present, u8p), self._hptr(paths), self._hptr(root))
        if at is None:
            check(self.lib.cstark_ledger_open_accounts(self.ctx, led, *out))
        else:
            check(self.lib.cstark_ledger_open_accounts_at(self.ctx, led, C.c_uint64(at), *out))
        return val, present.astype(bool), paths, root

    # ---- ledger checkpoints: ids are plain integers, 0 = the current state ----
    def ledger_checkpoint(self, led):
        cp = C.c_uint64(0)
        check(self.lib.cstark_ledger_checkpoint(self.ctx, led, C.byref(cp)))
        return cp.value

    def ledger_revert(self, led, cp):
        check(self.lib.cstark_ledger_revert(self.ctx, led, C.c_uint64(cp)))

    def ledger_release(self, led, cp):
        check(self.lib.cstark_ledger_release(self.ctx, led, C.c_uint64(cp)))

    def ledger_root_at(self, led, cp):
        root = np.zeros(7, np.uint64)
        check(self.lib.cstark_ledger_root_at(self.ctx, led, C.c_uint64(cp), self._hptr(root)))
        return root

    NODE_EMPTY, NODE_LEAF, NODE_INNER = 0, 1, 2   # cstark_ledger_node_kind

    def ledger_audit(self, led, cp=0):
        """cstark_ledger_audit: every stored node of the state at checkpoint cp (0: the current state) against its stored children, one
        launch -> _lib.LedgerAuditReportStruct (consistent, n_bad, first_kind / first_level / first_index, n_nodes, slots_*)"""
        report = _lib.LedgerAuditReportStruct()
        check(self.lib.cstark_ledger_audit(self.ctx, led, C.c_uint64(cp), C.byref(report)))
        return report

    PATH_VALID, PATH_INDEX_RANGE, PATH_LEAF, PATH_ROOT = 0, 1, 2, 3   # cstark_path_verdict

    def account_check_paths(self, indices, paths, roots, values=None, present=None, want_roots=False):
        """cstark_account_check_paths: folds every path ([count][depth + 1][7], any depth 1 .. 31) to a root on the device, one launch ->
        verdicts uint8[count] (cstark_path_verdict); with want_roots also the folded roots, uint64 [count][7], whatever the verdict.
        roots: one root [7] for all paths or one per path [count][7].  values [count][14] (and optionally present [count]): the leaf
        entry is checked against the account; without values the paths are paths of digests.  No ledger is needed and the resident
        witness is not touched."""
        idx = _np_u64(indices).reshape(-1)
        n = idx.size
        p = _np_u64(paths)
        if p.ndim != 3 or p.shape[0] != n or p.shape[2] != 7 or p.shape[1] < 2:
            raise ValueError("paths must be [count][depth + 1][7]")
        r = _np_u64(roots).reshape(-1, 7)
        val = None if values is None else _np_u64(values).reshape(-1, 14)
        if val is not None and val.shape[0] != n:
            raise ValueError("one 14-element value per path")
        if present is not None and val is None:
            raise ValueError("present without values")
        pres = None if present is None else np.ascontiguousarray(present, np.uint8).reshape(-1)
        if pres is not None and pres.size != n:
            raise ValueError("one present flag per path")
        verdicts = np.zeros(n, np.uint8)
        out = np.zeros((n, 7), np.uint64) if want_roots else None
        check(self.lib.cstark_account_check_paths(self.ctx, C.c_uint32(n), C.c_uint32(p.shape[1] - 1), self._hptr(idx),
                                                  None if val is None else self._hptr(val), None if pres is None else self._hptr(pres, u8p),
                                                  self._hptr(p), self._hptr(r), C.c_uint32(r.shape[0]), self._hptr(verdicts, u8p),
                                                  self._hptr(out) if want_roots else None))
        return (verdicts, out) if want_roots else verdicts

    # cstark_witness_verdict
    (WITNESS_VALID, WITNESS_INDEX_RANGE, WITNESS_SELF_TRANSFER, WITNESS_SENDER_LEAF, WITNESS_SENDER_PATH, WITNESS_BALANCE, WITNESS_MIDDLE_ROOT,
     WITNESS_RECEIVER_LEAF, WITNESS_NEXT_ROOT, WITNESS_SIGNATURE) = range(10)

    def tx_witness_check(self, metadata=None, final_root=None, check_signatures=False, want_folds=False):
        """cstark_tx_witness_check: is a transaction witness consistent?  One launch, one workgroup per transfer -> (report, verdicts)
        or, with want_folds, (report, verdicts, folds): report a _lib.WitnessReportStruct (n_tx, merkle_depth, first_bad (-1: none),
        first_verdict, n_bad, final_root[7] = the root the batch leaves, computed whatever the verdicts), verdicts uint8 [n_tx]
        (Backend.WITNESS_*, 0 = valid, the first test a transfer fails), folds uint64 [n_tx][4][7] (sender-old, sender-new,
        receiver-old, receiver-new).  metadata: any object with the TransactionMetadata arrays; it is checked in device scratch of its
        own and final_root must be None (the witness states its own).  metadata=None: the RESIDENT witness (upload_witness,
        ledger_apply) is checked where it lies against final_root, or without the last transfer's NEXT_ROOT test when that is None.
        check_signatures: every transfer's signature against the message its own row of the witness states.  Read-only: the resident
        witness and every ledger are as before, a proof after a check is the proof without it."""
        if metadata is None:
            n, arg, keep = self.n_tx, None, None
            root = None if final_root is None else _np_u64(final_root).reshape(7)
        else:
            if final_root is not None:
                raise ValueError("final_root is for the resident witness; a metadata object states its own")
            n, root = int(metadata.n_tx), None
            s, keep = self._witness_struct(metadata)
            arg = C.byref(s)
        report = _lib.WitnessReportStruct()
        verdicts = np.zeros(max(n, 1), np.uint8)
        folds = np.zeros((max(n, 1), 4, 7), np.uint64) if want_folds else None
        check(self.lib.cstark_tx_witness_check(self.ctx, arg, None if root is None else self._hptr(root),
                                               C.c_uint32(_lib.WITNESS_CHECK_SIGNATURES if check_signatures else 0), C.byref(report),
                                               self._hptr(verdicts, u8p), self._hptr(folds) if want_folds else None))
        verdicts = verdicts[:report.n_tx]
        return (report, verdicts, folds[:report.n_tx]) if want_folds else (report, verdicts)

    MULTI_VALID, MULTI_INDEX, MULTI_NODE_COUNT, MULTI_ROOT = 0, 1, 2, 3   # cstark_multi_verdict

    def account_multiproof_shape(self, depth, indices):
        """cstark_account_multiproof_shape (host only): -> (n_nodes, n_merges) of the multiproof of the strictly ascending `indices`"""
        idx = _np_u64(indices).reshape(-1)
        n_nodes, n_merges = C.c_uint32(0), C.c_uint32(0)
        check(self.lib.cstark_account_multiproof_shape(C.c_uint32(depth), C.c_uint32(idx.size), self._hptr(idx), C.byref(n_nodes), C.byref(n_merges)))
        return n_nodes.value, n_merges.value

    def ledger_open_multi(self, led, depth, indices, at=None):
        """cstark_ledger_open_multi: -> (values [count][14], present bool [count], nodes [n_nodes][7], root [7]): the accounts at the
        strictly ascending `indices` and ONE multiproof for all of them -- the de-duplicated siblings, level `depth` first and ascending
        within a level (include/cstark.h) -- under the current root, or with at=checkpoint id under the root of that checkpoint.
        Read-only: one gather, no hashing; the ledger and the resident witness are as before."""
        idx = _np_u64(indices).reshape(-1)
        n = idx.size
        need, _ = self.account_multiproof_shape(depth, idx)
        val, present = np.zeros((n, 14), np.uint64), np.zeros(n, np.uint8)
        nodes, root, n_nodes = np.zeros((need, 7), np.uint64), np.zeros(7, np.uint64), C.c_uint32(0)
        check(self.lib.cstark_ledger_open_multi(self.ctx, led, C.c_uint64(at or 0), C.c_uint32(n), self._hptr(idx), self._hptr(val),
                                                self._hptr(present, u8p), self._hptr(nodes) if need else None, C.c_uint32(need),
                                                C.byref(n_nodes), self._hptr(root)))
        assert n_nodes.value == need
        return val, present.astype(bool), nodes, root

    def account_check_multiproof(self, depth, indices, nodes, root, values=None, present=None, leaves=None):
        """cstark_account_check_multiproof: folds one multiproof (any depth 1 .. 31) on the device, the leaf hashes and then one launch
        per level -> (verdict, at, folded root [7], n_merges).  verdict: Backend.MULTI_* (0 = valid); INDEX (at = the first position
        whose index is out of range or not above its predecessor) and NODE_COUNT (at = the needed count) launch nothing, and the folded
        root is None for them (n_merges too for INDEX).  Exactly one of values [count][14] (optionally with present [count]) and
        leaves [count][7] (digest mode).  nodes: [n_nodes][7], or None for none.  No ledger is needed and the resident witness is not
        touched."""
        idx = _np_u64(indices).reshape(-1)
        n = idx.size
        val = None if values is None else _np_u64(values).reshape(-1, 14)
        lv = None if leaves is None else _np_u64(leaves).reshape(-1, 7)
        if (val is None) == (lv is None):
            raise ValueError("exactly one of values and leaves")
        if (val if lv is None else lv).shape[0] != n:
            raise ValueError("one value or leaf per index")
        if present is not None and val is None:
            raise ValueError("present without values")
        pres = None if present is None else np.ascontiguousarray(present, np.uint8).reshape(-1)
        if pres is not None and pres.size != n:
            raise ValueError("one present flag per index")
        nd = None if nodes is None else _np_u64(nodes).reshape(-1, 7)
        if nd is not None and nd.shape[0] == 0:
            nd = None
        r = _np_u64(root).reshape(7)
        verdict, at, n_merges = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
        out = np.zeros(7, np.uint64)
        check(self.lib.cstark_account_check_multiproof(self.ctx, C.c_uint32(depth), C.c_uint32(n), self._hptr(idx),
                                                       None if val is None else self._hptr(val), None if pres is None else self._hptr(pres, u8p),
                                                       None if lv is None else self._hptr(lv), None if nd is None else self._hptr(nd),
                                                       C.c_uint32(0 if nd is None else nd.shape[0]), self._hptr(r), C.byref(verdict), C.byref(at),
                                                       self._hptr(out), C.byref(n_merges)))
        launched = verdict.value in (self.MULTI_VALID, self.MULTI_ROOT)
        return verdict.value, at.value, out if launched else None, None if verdict.value == self.MULTI_INDEX else n_merges.value

    UPDATE_VALID, UPDATE_INDEX, UPDATE_NODE_COUNT, UPDATE_OLD_ROOT, UPDATE_NEW_ROOT = 0, 1, 2, 3, 4   # cstark_update_verdict

    def account_check_update(self, depth, indices, old_values, new_values, nodes, old_root, new_root=None, old_present=None, new_present=None):
        """cstark_account_check_update: folds one multi-opening over the old AND the new state of its accounts in one pass on the
        device, with the launches of one account_check_multiproof -> (verdict, at, new root [7], n_changed).  verdict: Backend.UPDATE_*
        (0 = valid); INDEX and NODE_COUNT as in account_check_multiproof (nothing launched, n_changed None); OLD_ROOT: the old values do
        not fold to old_root; NEW_ROOT: they do, and the new values fold to something other than new_root.  The new root is the fold of
        the new state for VALID and NEW_ROOT and None otherwise.  new_root=None: compute only.  old_present / new_present: [count],
        None for all present.  nodes: [n_nodes][7], or None for none.  No ledger is needed and the resident witness is not touched."""
        idx = _np_u64(indices).reshape(-1)
        n = idx.size
        old, new = _np_u64(old_values).reshape(-1, 14), _np_u64(new_values).reshape(-1, 14)
        if old.shape[0] != n or new.shape[0] != n:
            raise ValueError("one old and one new value per index")
        flags = []
        for present in (old_present, new_present):
            pres = None if present is None else np.ascontiguousarray(present, np.uint8).reshape(-1)
            if pres is not None and pres.size != n:
                raise ValueError("one present flag per index")
            flags.append(pres)
        nd = None if nodes is None else _np_u64(nodes).reshape(-1, 7)
        if nd is not None and nd.shape[0] == 0:
            nd = None
        r_old = _np_u64(old_root).reshape(7)
        r_new = None if new_root is None else _np_u64(new_root).reshape(7)
        verdict, at, n_changed = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
        out = np.zeros(7, np.uint64)
        check(self.lib.cstark_account_check_update(self.ctx, C.c_uint32(depth), C.c_uint32(n), self._hptr(idx), self._hptr(old),
                                                   None if flags[0] is None else self._hptr(flags[0], u8p), self._hptr(new),
                                                   None if flags[1] is None else self._hptr(flags[1], u8p), None if nd is None else self._hptr(nd),
                                                   C.c_uint32(0 if nd is None else nd.shape[0]), self._hptr(r_old),
                                                   None if r_new is None else self._hptr(r_new), C.byref(verdict), C.byref(at), self._hptr(out),
                                                   C.byref(n_changed)))
        launched = verdict.value not in (self.UPDATE_INDEX, self.UPDATE_NODE_COUNT)
        folded = verdict.value in (self.UPDATE_VALID, self.UPDATE_NEW_ROOT)
        return verdict.value, at.value, out if folded else None, n_changed.value if launched else None

    def ledger_apply(self, led, depth, s_indices, r_indices, deltas, sig_rx, sig_s, want_witness=True, check_signatures=False):
        """cstark_ledger_apply: -> (refused_at, reason, arrays).  Applied (refused_at == -1): the batch's witness is resident in this
        backend (build_trace / prove / air_prove follow without an upload) and arrays is the dict of its eleven fields (None with
        want_witness=False).  Refused: nothing changed, arrays is None.  check_signatures: cstark_ledger_apply_checked -- every
        transfer's signature is checked on the device before anything is applied (reason 5 at the first bad one)."""
        s, r, dl = _np_u64(s_indices).reshape(-1), _np_u64(r_indices).reshape(-1), _np_u64(deltas).reshape(-1)
        n = s.size
        rx = _np_u64(sig_rx).reshape(-1, 6)
        ss = np.ascontiguousarray(sig_s, np.uint8).reshape(-1, 32)
        if not (r.size == dl.size == rx.shape[0] == ss.shape[0] == n):
            raise ValueError("the transfer arrays state different numbers of transfers")
        arrays, out = None, None
        if want_witness:
            arrays = dict(initial_roots=np.zeros((n, 7), np.uint64), final_root=np.zeros(7, np.uint64),
                          s_old_values=np.zeros((n, 14), np.uint64), r_old_values=np.zeros((n, 14), np.uint64),
                          s_indices=np.zeros(n, np.uint64), r_indices=np.zeros(n, np.uint64),
                          s_paths=np.zeros((n, depth + 1, 7), np.uint64), r_paths=np.zeros((n, depth + 1, 7), np.uint64),
                          deltas=np.zeros(n, np.uint64), sig_rx=np.zeros((n, 6), np.uint64), sig_s=np.zeros((n, 32), np.uint8))
            st = _lib.TxWitnessStruct()
            st.n_tx, st.merkle_depth = n, depth
            for f, a in arrays.items():
                setattr(st, f, a.ctypes.data_as(u8p if f == "sig_s" else u64p))
            out = C.byref(st)
        at, reason = C.c_int32(-1), C.c_int32(0)
        apply = self.lib.cstark_ledger_apply_checked if check_signatures else self.lib.cstark_ledger_apply
        check(apply(self.ctx, led, C.c_uint32(n), self._hptr(s), self._hptr(r), self._hptr(dl), self._hptr(rx), self._hptr(ss, u8p),
                    out, C.byref(at), C.byref(reason)))
        if at.value >= 0:
            return at.value, reason.value, None
        self.resident = None   # an example that believed its own witness resident uploads again
        self.n_tx, self.depth = n, depth
        return -1, 0, arrays

    SELECT_CHECK_SIGNATURES, SELECT_POW2, SELECT_APPLY = 1, 2, 4   # CSTARK_SELECT_*

    def ledger_select(self, led, depth, s_indices, r_indices, deltas, sig_rx, sig_s, want, flags=0, chunk=0, want_messages=False, want_witness=True):
        """cstark_ledger_select: -> (status uint8 [n], selected uint32 [n_selected], messages [n][28] or None, report, arrays): the status
        of every candidate of the pool (cstark_ledger_reason, 8 = HELD, 9 = NOT_REACHED), the selected candidate numbers, and with
        SELECT_APPLY the witness of the applied selection (the dict of its eleven fields, None without want_witness or with nothing
        selected), which is then resident in this backend.  sig_rx / sig_s may be None without SELECT_CHECK_SIGNATURES and SELECT_APPLY."""
        s, r, dl = _np_u64(s_indices).reshape(-1), _np_u64(r_indices).reshape(-1), _np_u64(deltas).reshape(-1)
        n = s.size
        rx = None if sig_rx is None else _np_u64(sig_rx).reshape(-1, 6)
        ss = None if sig_s is None else np.ascontiguousarray(sig_s, np.uint8).reshape(-1, 32)
        if not (r.size == dl.size == n) or (rx is not None and rx.shape[0] != n) or (ss is not None and ss.shape[0] != n):
            raise ValueError("the candidate arrays state different numbers of candidates")
        cap = max(1, min(int(want), n))
        status, selected = np.zeros(n, np.uint8), np.zeros(cap, np.uint32)
        messages = np.zeros((n, 28), np.uint64) if want_messages else None
        arrays, out = None, None
        if (flags & self.SELECT_APPLY) and want_witness:
            arrays = dict(initial_roots=np.zeros((cap, 7), np.uint64), final_root=np.zeros(7, np.uint64),
                          s_old_values=np.zeros((cap, 14), np.uint64), r_old_values=np.zeros((cap, 14), np.uint64),
                          s_indices=np.zeros(cap, np.uint64), r_indices=np.zeros(cap, np.uint64),
                          s_paths=np.zeros((cap, depth + 1, 7), np.uint64), r_paths=np.zeros((cap, depth + 1, 7), np.uint64),
                          deltas=np.zeros(cap, np.uint64), sig_rx=np.zeros((cap, 6), np.uint64), sig_s=np.zeros((cap, 32), np.uint8))
            st = _lib.TxWitnessStruct()
            st.n_tx, st.merkle_depth = cap, depth
            for f, a in arrays.items():
                setattr(st, f, a.ctypes.data_as(u8p if f == "sig_s" else u64p))
            out = C.byref(st)
        report = _lib.LedgerSelectionStruct()
        check(self.lib.cstark_ledger_select(self.ctx, led, C.c_uint32(n), self._hptr(s), self._hptr(r), self._hptr(dl),
                                            None if rx is None else self._hptr(rx), None if ss is None else self._hptr(ss, u8p),
                                            C.c_uint32(want), C.c_uint32(flags), C.c_uint32(chunk), self._hptr(status, u8p),
                                            selected.ctypes.data_as(C.POINTER(C.c_uint32)), None if messages is None else self._hptr(messages),
                                            C.byref(report), out))
        m = report.n_selected
        if (flags & self.SELECT_APPLY) and m:
            self.resident = None   # as ledger_apply: the selection's witness is the resident one now
            self.n_tx, self.depth = m, depth
            if arrays is not None:
                arrays = {f: (a if f == "final_root" else a[:m].copy()) for f, a in arrays.items()}
        else:
            arrays = None
        return status, selected[:m].copy(), messages, report, arrays

    # ---- K2 / K3 ----
    def field_generator(self):
        self.lib.cstark_field_generator.restype = C.c_uint64
        return int(self.lib.cstark_field_generator())

    def field_lde_offset(self):
        self.lib.cstark_field_lde_offset.restype = C.c_uint64
        return int(self.lib.cstark_field_lde_offset())

    def interpolate_columns(self, evals, out=None):
        """evals: int64 [width, n] tensor (destroyed). Returns the coefficient tensor."""
        width, n = evals.shape
        if out is None:
            out = self.empty_u64(width, n)
        check(self.lib.cstark_interpolate_columns(self.ctx, self._ptr(evals), self._ptr(out), C.c_uint32(width),
                                                  C.c_uint32(n.bit_length() - 1)))
        return out

    def lde_columns(self, coeffs, log_blowup, offset=None, k0=0, nk=None, out=None):
        width, n = coeffs.shape
        nk = (1 << log_blowup) - k0 if nk is None else nk
        if out is None:
            out = self.empty_u64(nk, width, n)
        off = self.field_lde_offset() if offset is None else int(offset)
        check(self.lib.cstark_lde_columns(self.ctx, self._ptr(coeffs), self._ptr(out), C.c_uint32(width),
                                          C.c_uint32(n.bit_length() - 1), C.c_uint32(log_blowup), C.c_uint64(off),
                                          C.c_uint32(k0), C.c_uint32(nk)))
        return out

    def step_columns(self, evals, block_len, log_blowup, col0=0, ncols=None, offset=None, k0=0, nk=None, coeffs=None, lde=None):
        """Coefficients and extension of columns [col0, col0 + ncols) of evals (int64 [width, n]) that are constant over blocks of
        block_len rows: returns (coeffs [width, n], lde [nk, width, n]) with these columns filled as interpolate_columns and
        lde_columns fill them (the other columns are not written; evals' columns are destroyed where the shape takes those two calls)."""
        width, n = evals.shape
        ncols = width - col0 if ncols is None else ncols
        nk = (1 << log_blowup) - k0 if nk is None else nk
        if coeffs is None:
            coeffs = self.empty_u64(width, n)
        if lde is None:
            lde = self.empty_u64(nk, width, n)
        off = self.field_lde_offset() if offset is None else int(offset)
        check(self.lib.cstark_step_columns(self.ctx, self._ptr(evals), self._ptr(coeffs), self._ptr(lde), C.c_uint32(width),
                                           C.c_uint32(col0), C.c_uint32(ncols), C.c_uint32(n.bit_length() - 1),
                                           C.c_uint32(block_len), C.c_uint32(log_blowup), C.c_uint64(off), C.c_uint32(k0), C.c_uint32(nk)))
        return coeffs, lde

    def step2_columns(self, evals, block_len, split, log_blowup, col0=0, ncols=None, offset=None, k0=0, nk=None, coeffs=None, lde=None):
        """step_columns for columns that hold one value on rows [0, split) of every block of block_len rows and another on rows
        [split, block_len), 0 < split < block_len."""
        width, n = evals.shape
        ncols = width - col0 if ncols is None else ncols
        nk = (1 << log_blowup) - k0 if nk is None else nk
        if coeffs is None:
            coeffs = self.empty_u64(width, n)
        if lde is None:
            lde = self.empty_u64(nk, width, n)
        off = self.field_lde_offset() if offset is None else int(offset)
        check(self.lib.cstark_step2_columns(self.ctx, self._ptr(evals), self._ptr(coeffs), self._ptr(lde), C.c_uint32(width),
                                            C.c_uint32(col0), C.c_uint32(ncols), C.c_uint32(n.bit_length() - 1), C.c_uint32(block_len),
                                            C.c_uint32(split), C.c_uint32(log_blowup), C.c_uint64(off), C.c_uint32(k0), C.c_uint32(nk)))
        return coeffs, lde

    # ---- K4 / K5 ----
    def empty_u8(self, *shape):
        return torch.empty(shape, dtype=torch.uint8, device=self.device)

    def hash_rows_fn(self, hash_fn, lde, log_blowup, k0=0):
        """cstark_hash_rows_fn: row hashes with Blake3_256 (0) or Sha3_256 (1)"""
        nk, width, n = lde.shape
        leaves = self.empty_u8(n << log_blowup, 32)
        check(self.lib.cstark_hash_rows_fn(self.ctx, C.c_uint32(hash_fn), self._ptr(lde), self._ptr(leaves, u8p), C.c_uint32(width),
                                           C.c_uint32(n.bit_length() - 1), C.c_uint32(log_blowup), C.c_uint32(k0), C.c_uint32(nk)))
        return leaves

    def merkle_build_fn(self, hash_fn, nodes):
        check(self.lib.cstark_merkle_build_fn(self.ctx, C.c_uint32(hash_fn), self._ptr(nodes, u8p), C.c_uint32((nodes.shape[0] // 2).bit_length() - 1)))
        return nodes

    def hash_rows(self, lde, log_blowup, k0=0, leaves=None):
        """lde: [nk, width, n]. leaves: uint8 [(n << log_blowup), 32]; rows of cosets [k0, k0+nk) are written."""
        nk, width, n = lde.shape
        if leaves is None:
            leaves = torch.zeros((n << log_blowup, 32), dtype=torch.uint8, device=self.device)
        check(self.lib.cstark_hash_rows(self.ctx, self._ptr(lde), self._ptr(leaves, u8p), C.c_uint32(width),
                                        C.c_uint32(n.bit_length() - 1), C.c_uint32(log_blowup), C.c_uint32(k0), C.c_uint32(nk)))
        return leaves

    def merkle_build(self, nodes):
        """nodes: uint8 [2 L, 32] with the leaves in the upper half; filled in place, nodes[1] is the root."""
        L2 = nodes.shape[0]
        check(self.lib.cstark_merkle_build(self.ctx, self._ptr(nodes, u8p), C.c_uint32((L2 // 2).bit_length() - 1)))
        return nodes

    # ---- K6 / K7 ----
    def evaluate_transitions(self, lde, depth, log_blowup=3, k0=0):
        nk, width, n = lde.shape
        out = self.empty_u64(nk, _lib.TX_NUM_CONSTRAINTS, n)
        check(self.lib.cstark_tx_evaluate_transitions(self.ctx, self._ptr(lde), self._ptr(out), C.c_uint32(depth),
                                                      C.c_uint32(n.bit_length() - 1), C.c_uint32(log_blowup), C.c_uint32(k0), C.c_uint32(nk)))
        return out

    def evaluate_constraints(self, lde, coeffs, pub_inputs, depth, log_blowup=3, k0=0, out=None, input_is_lde=False):
        """coeffs: _lib.TxCoeffsStruct (or any ctypes struct of the same layout); pub_inputs: 4 uint64.
        input_is_lde: the table is the extension of columns of degree < n over all 8 cosets (cstark_tx_evaluate_constraints_lde:
        same output, degree-split evaluation)."""
        nk, width, n = lde.shape
        if out is None:
            out = self.empty_u64(nk, n)
        pub = (C.c_uint64 * 4)(*[int(v) for v in pub_inputs])
        if input_is_lde:
            assert k0 == 0 and nk == 8 and log_blowup == 3
            check(self.lib.cstark_tx_evaluate_constraints_lde(self.ctx, self._ptr(lde), C.byref(coeffs), pub, self._ptr(out), C.c_uint32(depth),
                                                              C.c_uint32(n.bit_length() - 1)))
            return out
        check(self.lib.cstark_tx_evaluate_constraints(self.ctx, self._ptr(lde), C.byref(coeffs), pub, self._ptr(out), C.c_uint32(depth),
                                                      C.c_uint32(n.bit_length() - 1), C.c_uint32(log_blowup), C.c_uint32(k0), C.c_uint32(nk)))
        return out

    def evaluate_constraints_ext(self, lde, coeff_sets, pub_inputs, depth, log_blowup=3, k0=0, input_is_lde=False):
        """The merged evaluations for 1..3 coefficient sets in one pass over the frame (cstark_tx_evaluate_constraints_ext):
        returns [m][nk][n].  input_is_lde: as for evaluate_constraints (cstark_tx_evaluate_constraints_ext_lde)."""
        nk, width, n = lde.shape
        m = len(coeff_sets)
        out = self.empty_u64(m, nk, n)
        arr = (type(coeff_sets[0]) * m)(*coeff_sets)
        pub = (C.c_uint64 * 4)(*[int(v) for v in pub_inputs])
        if input_is_lde:
            assert k0 == 0 and nk == 8 and log_blowup == 3
            check(self.lib.cstark_tx_evaluate_constraints_ext_lde(self.ctx, self._ptr(lde), arr, C.c_uint32(m), pub, self._ptr(out),
                                                                  C.c_uint32(depth), C.c_uint32(n.bit_length() - 1)))
            return out
        check(self.lib.cstark_tx_evaluate_constraints_ext(self.ctx, self._ptr(lde), arr, C.c_uint32(m), pub, self._ptr(out), C.c_uint32(depth),
                                                          C.c_uint32(n.bit_length() - 1), C.c_uint32(log_blowup), C.c_uint32(k0), C.c_uint32(nk)))
        return out

    # ---- standalone sub-AIRs (MerkleAir, RangeProofAir) ----
    AIR_TRANSACTION, AIR_MERKLE, AIR_SCHNORR, AIR_RANGE, AIR_RESCUE_CHAIN = 0, 1, 2, 3, 4

    def rescue_chain_build_trace(self, seed, chain_length):
        """cstark_rescue_chain_build_trace: 14 x 8 * chain_length (benches/rescue.rs:277-322); seed: 7 elements, memory form"""
        s = _np_u64(seed)
        out = self.empty_u64(14, 8 * chain_length)
        check(self.lib.cstark_rescue_chain_build_trace(self.ctx, self._hptr(s), C.c_uint32(chain_length), self._ptr(out)))
        return out

    def rescue_prove(self, options, seed, chain_length):
        """cstark_rescue_prove: complete RescueAir proof of a chain of `chain_length` hashes from `seed` (benches/rescue.rs:66-86)"""
        s = _np_u64(seed)
        o = self._options_struct(options)
        self.lib.cstark_tx_proof_size_bound.restype = C.c_size_t
        cap = 2 * self.lib.cstark_tx_proof_size_bound(C.c_uint32(max(1, chain_length // 128)), C.byref(o))
        buf = (C.c_uint8 * cap)()
        n = C.c_size_t(0)
        check(self.lib.cstark_rescue_prove(self.ctx, C.byref(o), self._hptr(s), C.c_uint32(chain_length), buf, C.c_size_t(cap), C.byref(n)))
        return bytes(memoryview(buf)[:n.value])

    def merkle_build_trace(self):
        out = self.empty_u64(65, self.n_tx * 512)
        check(self.lib.cstark_merkle_build_trace(self.ctx, self._ptr(out)))
        return out

    def range_build_trace(self, number_mont):
        out = self.empty_u64(2, 64)
        check(self.lib.cstark_range_build_trace(self.ctx, C.c_uint64(int(number_mont)), self._ptr(out)))
        return out

    def range_build_trace_bits(self, words, log_n):
        """cstark_range_build_trace_bits: the synthetic long accumulator (2 x 2^log_n); returns (trace, V mod p in memory form)."""
        w = _np_u64(words)
        out = self.empty_u64(2, 1 << log_n)
        num = C.c_uint64()
        check(self.lib.cstark_range_build_trace_bits(self.ctx, w.ctypes.data_as(u64p), C.c_uint32(log_n), self._ptr(out), C.byref(num)))
        return out, num.value

    def range_prove_bits(self, options, words, log_n):
        """cstark_range_prove_bits: complete RangeProofAir proof over 2^log_n rows."""
        w = _np_u64(words)
        o = _lib.OptionsStruct(options.num_queries, options.blowup_factor, options.grinding_factor, options.hash_fn,
                               options.field_extension, options.fri_folding_factor, options.fri_max_remainder)
        self.lib.cstark_tx_proof_size_bound.restype = C.c_size_t
        cap = 2 * self.lib.cstark_tx_proof_size_bound(C.c_uint32(max(1, (1 << log_n) // 1024)), C.byref(o))
        buf = (C.c_uint8 * cap)()
        n = C.c_size_t(0)
        check(self.lib.cstark_range_prove_bits(self.ctx, C.byref(o), w.ctypes.data_as(u64p), C.c_uint32(log_n), buf, C.c_size_t(cap), C.byref(n)))
        return bytes(memoryview(buf)[:n.value])

    def range_prove_batch(self, options, numbers):
        """cstark_range_prove_batch: one reference-shaped (64-row) range proof per element of `numbers` (memory form).  Returns a
        sequence of proofs (bytes on access: the call itself leaves them in one host buffer)."""
        nums = _np_u64(numbers)
        o = self._options_struct(options)
        self.lib.cstark_tx_proof_size_bound.restype = C.c_size_t
        stride = int(self.lib.cstark_tx_proof_size_bound(C.c_uint32(1), C.byref(o)))
        buf = np.empty(nums.size * stride, np.uint8)
        lens = np.zeros(nums.size, np.uint64)
        check(self.lib.cstark_range_prove_batch(self.ctx, C.byref(o), self._hptr(nums), C.c_uint32(nums.size), buf.ctypes.data_as(u8p), C.c_size_t(stride),
                                                lens.ctypes.data_as(C.POINTER(C.c_size_t))))
        return ProofBatch(buf, stride, lens)

    @staticmethod
    def _hptr(a, typ=u64p):
        return a.ctypes.data_as(typ)

    def air_shape(self, air, n_items=2):
        w, nc, na, lce = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_uint32()
        check(self.lib.cstark_air_shape(C.c_int(air), C.c_uint32(n_items), C.byref(w), C.byref(nc), C.byref(na), C.byref(lce)))
        return w.value, nc.value, na.value, lce.value

    def air_validate_trace(self, air, trace, depth=0, public_inputs=None, want_cycles=False, want_frame=False):
        """cstark_air_validate_trace: every transition constraint on every frame of the device trace [width][n] and, with public_inputs
        (14 words, memory form; RangeProofAir: the number; SchnorrAir: anything but None), the boundary entries.  Returns a TraceReport."""
        assert trace.dim() == 2 and trace.dtype == torch.int64
        n = trace.shape[1]
        assert n > 0 and n & (n - 1) == 0, "the trace length must be a power of two"
        width, nc, cyc = _lib.air_trace_shape(air, n.bit_length() - 1)   # refuses an unknown AIR or an impossible length
        assert trace.shape[0] == width
        pub = None
        if public_inputs is not None:
            pub = np.zeros(14, np.uint64)
            flat = _np_u64(public_inputs).reshape(-1)[:14]
            pub[:flat.size] = flat
        codes = np.empty(n // cyc, np.uint32) if want_cycles else None
        frame = np.zeros(nc, np.uint64) if want_frame else None
        rep = _lib.TraceReportStruct()
        check(self.lib.cstark_air_validate_trace(self.ctx, C.c_int(air), self._ptr(trace), C.c_uint32(n.bit_length() - 1), C.c_uint32(depth),
                                                 self._hptr(pub) if pub is not None else None, C.byref(rep),
                                                 codes.ctypes.data_as(C.POINTER(C.c_uint32)) if want_cycles else None,
                                                 self._hptr(frame) if want_frame else None))
        return TraceReport(air, n, rep, codes, frame)

    def air_evaluate_transitions(self, air, lde, depth, log_blowup, k0=0):
        nk, width, n = lde.shape
        nc = self.air_shape(air)[1]
        out = self.empty_u64(nk, nc, n)
        check(self.lib.cstark_air_evaluate_transitions(self.ctx, C.c_int(air), self._ptr(lde), self._ptr(out), C.c_uint32(depth),
                                                       C.c_uint32(n.bit_length() - 1), C.c_uint32(log_blowup), C.c_uint32(k0), C.c_uint32(nk)))
        return out

    def air_combine(self, air, lde, evals, t_alpha, t_beta, b_alpha, b_beta, assertion_values, log_blowup, k0=0, n_items=2, avals_lde=None):
        nk, width, n = lde.shape
        out = self.empty_u64(nk, n)
        arrs = [_np_u64(a) for a in (t_alpha, t_beta, b_alpha, b_beta)]
        av = None if assertion_values is None else _np_u64(assertion_values)
        check(self.lib.cstark_air_combine(self.ctx, C.c_int(air), C.c_uint32(n_items), self._ptr(lde), self._ptr(evals),
                                          *[a.ctypes.data_as(u64p) for a in arrs], None if av is None else av.ctypes.data_as(u64p),
                                          None if avals_lde is None else self._ptr(avals_lde), C.c_uint32(0 if avals_lde is None else avals_lde.shape[1]),
                                          self._ptr(out), C.c_uint32(n.bit_length() - 1), C.c_uint32(log_blowup), C.c_uint32(k0), C.c_uint32(nk)))
        return out

    def merkle_evaluate_constraints(self, lde, depth, t_alpha, t_beta, b_alpha, b_beta, assertion_values, log_blowup, k0=0):
        """MerkleAir's combined constraint evaluations through the fused evaluator (cstark_merkle_evaluate_constraints)."""
        nk, width, n = lde.shape
        out = self.empty_u64(nk, n)
        arrs = [_np_u64(a) for a in (t_alpha, t_beta, b_alpha, b_beta, assertion_values)]
        check(self.lib.cstark_merkle_evaluate_constraints(self.ctx, C.c_uint32(depth), self._ptr(lde), *[a.ctypes.data_as(u64p) for a in arrs],
                                                          self._ptr(out), C.c_uint32(n.bit_length() - 1), C.c_uint32(log_blowup), C.c_uint32(k0),
                                                          C.c_uint32(nk)))
        return out

    def schnorr_evaluate_constraints(self, lde, aux_lde, t_alpha, t_beta, b_alpha, b_beta, avals_lde, log_blowup, k0=0, n_sig=2):
        """SchnorrAir's combined constraint evaluations through the fused evaluator (cstark_schnorr_evaluate_constraints)."""
        nk, width, n = lde.shape
        out = self.empty_u64(nk, n)
        arrs = [_np_u64(a) for a in (t_alpha, t_beta, b_alpha, b_beta)]
        check(self.lib.cstark_schnorr_evaluate_constraints(self.ctx, C.c_uint32(n_sig), self._ptr(lde), self._ptr(aux_lde),
                                                           *[a.ctypes.data_as(u64p) for a in arrs], self._ptr(avals_lde),
                                                           C.c_uint32(avals_lde.shape[1]), self._ptr(out), C.c_uint32(n.bit_length() - 1),
                                                           C.c_uint32(log_blowup), C.c_uint32(k0), C.c_uint32(nk)))
        return out

    # ---- standalone SchnorrAir ----
    def schnorr_evaluate_constraints_lde(self, lde, aux_lde, t_alpha, t_beta, b_alpha, b_beta, avals_lde, n_sig=2):
        """cstark_schnorr_evaluate_constraints_lde: all 8 cosets of genuine extensions -> the degree-split evaluation of the curve gadgets"""
        nk, width, n = lde.shape
        assert nk == 8 and width == 56
        out = self.empty_u64(8, n)
        arrs = [_np_u64(a) for a in (t_alpha, t_beta, b_alpha, b_beta)]
        check(self.lib.cstark_schnorr_evaluate_constraints_lde(self.ctx, C.c_uint32(n_sig), self._ptr(lde), self._ptr(aux_lde), *[a.ctypes.data_as(u64p) for a in arrs],
                                                               self._ptr(avals_lde), C.c_uint32(avals_lde.shape[1]), self._ptr(out), C.c_uint32(n.bit_length() - 1)))
        return out

    def upload_schnorr_witness(self, messages, sig_rx, sig_s):
        self.resident = None
        m, rx = _np_u64(messages), _np_u64(sig_rx)
        s = np.ascontiguousarray(sig_s, np.uint8)
        n_sig = m.shape[0]
        check(self.lib.cstark_schnorr_witness_upload(self.ctx, C.c_uint32(n_sig), m.ctypes.data_as(u64p), rx.ctypes.data_as(u64p),
                                                     s.ctypes.data_as(u8p)))
        self.n_tx = n_sig

    SIG_VALID, SIG_MISMATCH, SIG_KEY_NOT_ON_CURVE, SIG_SCALAR_RANGE = 0, 1, 2, 3   # cstark_sig_verdict

    def schnorr_check(self, messages, sig_rx, sig_s, want_rx=False):
        """cstark_schnorr_check_signatures: verify_signature for every (message [28], R.x [6], s [32]) on the device -> verdicts
        uint8[count] (cstark_sig_verdict); with want_rx also the affine x of s*G + h*P, uint64 [count][6].  The resident witness is
        not touched."""
        m, rx = _np_u64(messages).reshape(-1, 28), _np_u64(sig_rx).reshape(-1, 6)
        s = np.ascontiguousarray(sig_s, np.uint8).reshape(-1, 32)
        n = m.shape[0]
        if not (rx.shape[0] == s.shape[0] == n):
            raise ValueError("the signature arrays state different numbers of signatures")
        verdicts = np.zeros(n, np.uint8)
        x = np.zeros((n, 6), np.uint64) if want_rx else None
        check(self.lib.cstark_schnorr_check_signatures(self.ctx, C.c_uint32(n), self._hptr(m), self._hptr(rx), self._hptr(s, u8p),
                                                       self._hptr(verdicts, u8p), self._hptr(x) if want_rx else None))
        return (verdicts, x) if want_rx else verdicts

    # cstark_sign_status.  A signer for building batches, tests and benchmarks (small integer keys): it is not a wallet.
    SIGN_OK, SIGN_NEGATIVE, SIGN_RANGE, SIGN_INFINITY, SIGN_EXHAUSTED = 0, 1, 2, 3, 4
    SIG_MAX_SECRET = 255

    def schnorr_public_keys(self, secrets):
        """cstark_schnorr_public_keys: secrets[i] * G for secrets in 1 .. 255 -> uint64 [count][12], affine (x, y) in memory form"""
        sk = _np_u64(secrets).reshape(-1)
        keys = np.zeros((sk.size, 12), np.uint64)
        check(self.lib.cstark_schnorr_public_keys(self.ctx, C.c_uint32(sk.size), self._hptr(sk), self._hptr(keys)))
        return keys

    @staticmethod
    def _sign_inputs(messages, secrets):
        m, sk = _np_u64(messages).reshape(-1, 28), _np_u64(secrets).reshape(-1)
        if m.shape[0] != sk.size:
            raise ValueError("the signing arrays state different numbers of signatures")
        return m, sk, np.zeros((sk.size, 6), np.uint64), np.zeros((sk.size, 32), np.uint8), np.zeros(sk.size, np.uint8)

    def schnorr_sign_nonces(self, messages, secrets, nonces):
        """cstark_schnorr_sign_nonces: one signing attempt per entry with the caller's nonce (uint64 [count][5] little-endian limbs,
        below 2^264) -> (sig_rx [count][6], sig_s [count][32], status uint8 [count]); every output is defined whatever the status."""
        m, sk, rx, s, status = self._sign_inputs(messages, secrets)
        r = _np_u64(nonces).reshape(-1, 5)
        if r.shape[0] != sk.size:
            raise ValueError("the signing arrays state different numbers of signatures")
        check(self.lib.cstark_schnorr_sign_nonces(self.ctx, C.c_uint32(sk.size), self._hptr(m), self._hptr(sk), self._hptr(r), self._hptr(rx),
                                                  self._hptr(s, u8p), self._hptr(status, u8p)))
        return rx, s, status

    def schnorr_sign(self, messages, secrets, seed=0, max_attempts=256):
        """cstark_schnorr_sign: the seeded signer -> (sig_rx, sig_s, attempts uint32 [count], status uint8 [count]); the result of a
        signature is that of the first accepted attempt of its own nonce stream, SIGN_EXHAUSTED (zero outputs) without one."""
        m, sk, rx, s, status = self._sign_inputs(messages, secrets)
        attempts = np.zeros(sk.size, np.uint32)
        check(self.lib.cstark_schnorr_sign(self.ctx, C.c_uint32(sk.size), self._hptr(m), self._hptr(sk), C.c_uint64(seed), C.c_uint32(max_attempts),
                                           self._hptr(rx), self._hptr(s, u8p), self._hptr(attempts, C.POINTER(C.c_uint32)), self._hptr(status, u8p)))
        return rx, s, attempts, status

    def ledger_messages(self, led, s_indices, r_indices, deltas):
        """cstark_ledger_messages: -> (refused_at, reason, messages [n_tx][28]): what each transfer of the batch has to sign, or the
        refusal cstark_ledger_apply would give (messages is None then).  Read-only."""
        s, r, dl = _np_u64(s_indices).reshape(-1), _np_u64(r_indices).reshape(-1), _np_u64(deltas).reshape(-1)
        if not (r.size == dl.size == s.size):
            raise ValueError("the transfer arrays state different numbers of transfers")
        out = np.zeros((s.size, 28), np.uint64)
        at, reason = C.c_int32(-1), C.c_int32(0)
        check(self.lib.cstark_ledger_messages(self.ctx, led, C.c_uint32(s.size), self._hptr(s), self._hptr(r), self._hptr(dl), self._hptr(out),
                                              C.byref(at), C.byref(reason)))
        return at.value, reason.value, out if at.value < 0 else None

    def ledger_sign(self, led, s_indices, r_indices, deltas, secrets, seed=0, max_attempts=256):
        """cstark_ledger_sign: -> (refused_at, reason, sig_rx, sig_s, attempts); refused (reason 7: a secret is not its sender's key, or
        a reason of cstark_ledger_apply): the three arrays are None.  Read-only."""
        s, r, dl, sk = (_np_u64(a).reshape(-1) for a in (s_indices, r_indices, deltas, secrets))
        n = s.size
        if not (r.size == dl.size == sk.size == n):
            raise ValueError("the transfer arrays state different numbers of transfers")
        rx, ss, attempts = np.zeros((n, 6), np.uint64), np.zeros((n, 32), np.uint8), np.zeros(n, np.uint32)
        at, reason = C.c_int32(-1), C.c_int32(0)
        check(self.lib.cstark_ledger_sign(self.ctx, led, C.c_uint32(n), self._hptr(s), self._hptr(r), self._hptr(dl), self._hptr(sk), C.c_uint64(seed),
                                          C.c_uint32(max_attempts), self._hptr(rx), self._hptr(ss, u8p), self._hptr(attempts, C.POINTER(C.c_uint32)),
                                          C.byref(at), C.byref(reason)))
        if at.value >= 0:
            return at.value, reason.value, None, None, None
        return -1, 0, rx, ss, attempts

    def schnorr_build_trace(self):
        out = self.empty_u64(56, self.n_tx * 512)
        check(self.lib.cstark_schnorr_build_trace(self.ctx, self._ptr(out)))
        return out

    def schnorr_aux_columns(self):
        out = self.empty_u64(19, self.n_tx * 512)
        check(self.lib.cstark_schnorr_aux_columns(self.ctx, self._ptr(out)))
        return out

    def schnorr_evaluate_transitions(self, lde, aux_lde, log_blowup, k0=0):
        nk, width, n = lde.shape
        out = self.empty_u64(nk, 56, n)
        check(self.lib.cstark_schnorr_evaluate_transitions(self.ctx, self._ptr(lde), self._ptr(aux_lde), self._ptr(out),
                                                           C.c_uint32(n.bit_length() - 1), C.c_uint32(log_blowup), C.c_uint32(k0), C.c_uint32(nk)))
        return out

    # ---- measurement ----
    CE_PARTS = ("rounds", "dbl_sG", "add_sG", "dbl_hP", "add_hP", "final_add", "lin_a", "lin_b", "lin_c")

    def set_part_timing(self, enable=True):
        check(self.lib.cstark_ctx_set_part_timing(self.ctx, C.c_int(1 if enable else 0)))

    def constraint_part_ms(self):
        ms = (C.c_float * 9)()
        check(self.lib.cstark_tx_constraint_part_ms(self.ctx, ms))
        return dict(zip(self.CE_PARTS, [float(v) for v in ms]))

    def lde_timing_ms(self):
        """(milliseconds, evaluations written) of all low-degree extensions since the last call (part timing on)"""
        ms, el = C.c_float(), C.c_uint64()
        check(self.lib.cstark_lde_timing_ms(self.ctx, C.byref(ms), C.byref(el)))
        return float(ms.value), int(el.value)

    def schnorr_assertion_polys(self, log_n):
        out = self.empty_u64(12, 1 << log_n)
        check(self.lib.cstark_schnorr_assertion_polys(self.ctx, self._ptr(out), C.c_uint32(log_n)))
        return out

    # ---- composition polynomial ----
    def composition_columns(self, combined, out=None):
        b, n = combined.shape
        if out is None:
            out = self.empty_u64(b, n)
        check(self.lib.cstark_composition_columns(self.ctx, self._ptr(combined), self._ptr(out), C.c_uint32(n.bit_length() - 1),
                                                  C.c_uint32(b.bit_length() - 1)))
        return out

    # ---- out-of-domain frame + DEEP composition ----
    def evaluate_polys_at(self, coeffs, points):
        width, n = coeffs.shape
        pts = _np_u64(points)
        out = np.zeros((pts.size, width), np.uint64)
        check(self.lib.cstark_evaluate_polys_at(self.ctx, self._ptr(coeffs), C.c_uint32(width), C.c_uint32(n.bit_length() - 1),
                                                pts.ctypes.data_as(u64p), C.c_uint32(pts.size), out.ctypes.data_as(u64p)))
        return out

    def deep_composition(self, trace_lde, comp_lde, z, ood_trace, ood_comp, alpha, beta, delta, deg_a, deg_b, log_blowup, k0=0, out=None):
        nk, width, n = trace_lde.shape
        nb = comp_lde.shape[1]
        if out is None:
            out = self.empty_u64(nk, n)
        arrs = [_np_u64(a) for a in (ood_trace, ood_comp, alpha, beta, delta)]
        check(self.lib.cstark_deep_composition(self.ctx, self._ptr(trace_lde), self._ptr(comp_lde), C.c_uint32(width), C.c_uint32(nb),
                                               C.c_uint64(int(z)), *[a.ctypes.data_as(u64p) for a in arrs], C.c_uint64(int(deg_a)),
                                               C.c_uint64(int(deg_b)), self._ptr(out), C.c_uint32(n.bit_length() - 1), C.c_uint32(log_blowup),
                                               C.c_uint32(k0), C.c_uint32(nk)))
        return out

    def evaluate_polys_at_ext(self, coeffs, z):
        """cstark_evaluate_polys_at_ext: base-field coefficient columns at one point of the degree-m extension (z: m memory-form
        words); returns a host [width][m] array"""
        width, n = coeffs.shape
        m = len(z)
        zp = (C.c_uint64 * m)(*[int(v) for v in z])
        out = np.zeros((width, m), np.uint64)
        check(self.lib.cstark_evaluate_polys_at_ext(self.ctx, self._ptr(coeffs), C.c_uint32(width), C.c_uint32(n.bit_length() - 1), C.c_uint32(m),
                                                    zp, out.ctypes.data_as(u64p)))
        return out

    def deep_composition_ext(self, trace_lde, comp_lde, z, ood_trace, ood_comp, alpha, beta, delta, deg_a, deg_b, log_blowup, out=None):
        """cstark_deep_composition_ext: trace_lde [b][width][n], comp_lde [b][m nb][n] (column m i + q = component q of composition
        column i); z, deg_a, deg_b: m words; ood_trace [2][width][m], ood_comp [nb][m], alpha, beta [width][m], delta [nb][m].
        Returns [m][b][n], component-major."""
        b, width, n = trace_lde.shape
        m = len(z)
        nb = comp_lde.shape[1] // m
        assert b == 1 << log_blowup and comp_lde.shape[0] == b and comp_lde.shape[1] == m * nb
        if out is None:
            out = self.empty_u64(m, b, n)
        arrs = [_np_u64(a) for a in (z, ood_trace, ood_comp, alpha, beta, delta, deg_a, deg_b)]
        assert [a.size for a in arrs] == [m, 2 * width * m, nb * m, width * m, width * m, nb * m, m, m]
        check(self.lib.cstark_deep_composition_ext(self.ctx, self._ptr(trace_lde), self._ptr(comp_lde), C.c_uint32(width), C.c_uint32(nb), C.c_uint32(m),
                                                   *[a.ctypes.data_as(u64p) for a in arrs], self._ptr(out), C.c_uint32(n.bit_length() - 1),
                                                   C.c_uint32(log_blowup)))
        return out

    # ---- FRI ----
    def interleave_cosets(self, coset_major):
        b, n = coset_major.shape
        out = self.empty_u64(b * n)
        check(self.lib.cstark_interleave_cosets(self.ctx, self._ptr(coset_major), self._ptr(out), C.c_uint32(n.bit_length() - 1),
                                                C.c_uint32(b.bit_length() - 1)))
        return out

    def fri_fold4(self, evals, offset, alpha):
        N = evals.numel()
        out = self.empty_u64(N // 4)
        check(self.lib.cstark_fri_fold4(self.ctx, self._ptr(evals), self._ptr(out), C.c_uint32(N.bit_length() - 1), C.c_uint64(int(offset)),
                                        C.c_uint64(int(alpha))))
        return out

    def fri_fold(self, evals, offset, alpha, folding=4):
        """cstark_fri_fold: one FRI layer with folding factor 4, 8 or 16"""
        N = evals.numel()
        out = self.empty_u64(N // folding)
        check(self.lib.cstark_fri_fold(self.ctx, self._ptr(evals), self._ptr(out), C.c_uint32(N.bit_length() - 1), C.c_uint32(folding),
                                       C.c_uint64(int(offset)), C.c_uint64(int(alpha))))
        return out

    def fri_fold_ext(self, evals, offset, alpha, folding=4):
        """cstark_fri_fold_ext: evals [m][N] component-major, alpha: m memory-form words"""
        m, N = evals.shape
        out = self.empty_u64(m, N // folding)
        al = (C.c_uint64 * m)(*[int(v) for v in alpha])
        check(self.lib.cstark_fri_fold_ext(self.ctx, self._ptr(evals), self._ptr(out), C.c_uint32(N.bit_length() - 1), C.c_uint32(folding),
                                           C.c_uint64(int(offset)), C.c_uint32(m), al))
        return out

    def fri_commit_layer(self, evals, folding=4):
        """Merkle tree over the rows { e[i + t N/f] } of a layer; returns the node array (nodes[1] = root)."""
        N = evals.numel()
        q = N // folding
        nodes = torch.zeros((2 * q, 32), dtype=torch.uint8, device=self.device)
        self.hash_rows(evals.view(1, folding, q), 0, leaves=nodes[q:])
        self.merkle_build(nodes)
        return nodes

    # ---- whole proof -------------------------------------------------------------------------------------------
    def prove(self, options):
        """cstark_tx_prove on the uploaded witness; `options` has the 7 ProofOptions attributes.  Returns proof bytes."""
        o = _lib.OptionsStruct(options.num_queries, options.blowup_factor, options.grinding_factor, options.hash_fn,
                               options.field_extension, options.fri_folding_factor, options.fri_max_remainder)
        self.lib.cstark_tx_proof_size_bound.restype = C.c_size_t
        cap = self.lib.cstark_tx_proof_size_bound(C.c_uint32(self.n_tx), C.byref(o))
        buf = self._proof_buffer(cap)
        n = C.c_size_t(0)
        check(self.lib.cstark_tx_prove(self.ctx, C.byref(o), buf, C.c_size_t(cap), C.byref(n)))
        return bytes(memoryview(buf)[:n.value])

    def _proof_buffer(self, cap):
        """host buffer the library writes a proof into, kept across calls (a fresh ctypes array is zero-filled: 1 MB per proof)"""
        if getattr(self, "_pbuf_cap", 0) < cap:
            self._pbuf, self._pbuf_cap = (C.c_uint8 * cap)(), cap
        return self._pbuf

    # ---- one proof across several GPUs by LDE coset: the phases of cstark_tx_shard_* (driver: sharding.prove_sharded) -------------
    def _options_struct(self, options):
        return _lib.OptionsStruct(options.num_queries, options.blowup_factor, options.grinding_factor, options.hash_fn,
                                  options.field_extension, options.fri_folding_factor, options.fri_max_remainder)

    def shard_commit(self, options, k0, nk):
        """phase 1 -> the roots of this rank's subtrees (its nk leaves of every row), uint8 [1][n][32]"""
        self._shard_options = options
        n = self.n_tx * _lib.TX_CYCLE_LENGTH
        leaves = self.empty_u8(1, n, 32)
        o = self._options_struct(options)
        check(self.lib.cstark_tx_shard_commit(self.ctx, C.byref(o), C.c_uint32(k0), C.c_uint32(nk), self._ptr(leaves, u8p)))
        self._shard_nk = nk
        return leaves

    def shard_evaluate(self, leaves_all):
        """phase 2: all-gathered subtree roots [W][n][32] -> this rank's share of the merged constraint evaluations, int64 [R][n]
        (R = cstark_tx_shard_rows(nk): its cosets, or its even cosets + its share of the four odd ones; include/cstark.h)"""
        n = self.n_tx * _lib.TX_CYCLE_LENGTH
        assert tuple(leaves_all.shape) == (8 // self._shard_nk, n, 32) and leaves_all.dtype == torch.uint8
        self.lib.cstark_tx_shard_rows.restype = C.c_uint32
        out = self.empty_u64(int(self.lib.cstark_tx_shard_rows(C.c_uint32(self._shard_nk))), n)
        check(self.lib.cstark_tx_shard_evaluate(self.ctx, self._ptr(leaves_all.contiguous(), u8p), self._ptr(out), C.c_uint32(out.shape[0])))
        return out

    def shard_compose(self, combined_all):
        """phase 3 (the rank that owns coset 0): the ranks' shares [W * R][n] -> query positions, int32 [num_queries]"""
        nq = self._shard_options.num_queries
        pos = np.zeros(nq, np.uint32)
        n = self.n_tx * _lib.TX_CYCLE_LENGTH
        assert combined_all.dim() == 2 and combined_all.shape[1] == n
        check(self.lib.cstark_tx_shard_compose(self.ctx, self._ptr(combined_all.contiguous()), C.c_uint32(combined_all.shape[0]),
                                               pos.ctypes.data_as(C.POINTER(C.c_uint32))))
        return torch.from_numpy(pos.view(np.int32)).to(self.device)

    def shard_open_rows(self, positions):
        """phase 4: rows of the extended trace at `positions` that lie in this rank's cosets, each with the bottom log2(nk) siblings of
        its authentication path (zeros elsewhere), int64 [nq][94 + 4 log2(nk)]"""
        pos = np.ascontiguousarray(positions.detach().cpu().numpy().view(np.uint32))
        self.lib.cstark_tx_shard_open_words.restype = C.c_uint32
        rows = self.empty_u64(pos.size, int(self.lib.cstark_tx_shard_open_words(C.c_uint32(self._shard_nk))))
        check(self.lib.cstark_tx_shard_open_rows(self.ctx, pos.ctypes.data_as(C.POINTER(C.c_uint32)), C.c_uint32(pos.size), self._ptr(rows)))
        return rows

    def shard_finish(self, rows):
        """phase 5 (the rank that ran phase 3): complete opened rows -> proof bytes"""
        o = self._options_struct(self._shard_options)
        self.lib.cstark_tx_proof_size_bound.restype = C.c_size_t
        cap = self.lib.cstark_tx_proof_size_bound(C.c_uint32(self.n_tx), C.byref(o))
        buf = (C.c_uint8 * cap)()
        n = C.c_size_t(0)
        check(self.lib.cstark_tx_shard_finish(self.ctx, self._ptr(rows.contiguous()), buf, C.c_size_t(cap), C.byref(n)))
        return bytes(memoryview(buf)[:n.value])

    PROVE_STAGES = ("trace", "interpolate", "lde", "commit", "constraints", "composition", "ood", "deep", "fri", "queries")

    def prove_stage_ms(self):
        ms = (C.c_float * len(self.PROVE_STAGES))()
        check(self.lib.cstark_prove_stage_ms(self.ctx, ms))
        return dict(zip(self.PROVE_STAGES, [float(v) for v in ms]))

    PROOF_FORMS = ("plain", "compact")

    @property
    def proof_form(self):
        """cstark_ctx_proof_form / cstark_ctx_set_proof_form: "plain" (the default: one authentication path per opened row) or "compact"
        (one Merkle multiproof per tree) -- the form every single-GPU prover of this backend writes; the sharded phases refuse "compact"."""
        f = C.c_uint32(0)
        check(self.lib.cstark_ctx_proof_form(self.ctx, C.byref(f)))
        return self.PROOF_FORMS[f.value]

    @proof_form.setter
    def proof_form(self, form):
        if form not in self.PROOF_FORMS:
            raise ValueError("proof_form is 'plain' or 'compact', not %r" % (form,))
        check(self.lib.cstark_ctx_set_proof_form(self.ctx, C.c_uint32(self.PROOF_FORMS.index(form))))

    def prove_channel(self):
        """cstark_prove_channel: "device" when the Fiat-Shamir channel of the last proof ran on the GPU (the host waited once), "host" when
        the host absorbed and drew between the stages (Sha3 coin, proof of work, sharded proofs, CSTARK_HOST_CHANNEL=1)"""
        ch = C.c_uint32(0)
        check(self.lib.cstark_prove_channel(self.ctx, C.byref(ch)))
        return ("host", "device")[ch.value]

    # ---- verification (cstark_tx_verify) ---------------------------------------------------------------------------------------
    def tx_verify(self, proofs, initial_roots, final_roots, options=None):
        """TransactionExample::verify for a list of proofs (bytes) or a ProofBatch, in one call.  initial_roots / final_roots: [count][7]
        (or [7] for every proof), memory form.  options: None = each proof's own options, else every proof must state exactly these.
        Returns the verdicts, int32 [count] (0 = accepted; names: certificate_stark_amd.VERDICTS)."""
        return self._tx_call(self.lib.cstark_tx_verify, proofs, initial_roots, final_roots, options)

    def _tx_call(self, fn, proofs, initial_roots, final_roots, options, convert=None):
        """cstark_tx_verify, or cstark_tx_convert with convert = _Conversion: the arguments the two share"""
        count = len(proofs)
        verdicts = np.zeros(count, np.int32)
        vp = verdicts.ctypes.data_as(C.POINTER(C.c_int32))
        if count == 0:
            check(fn(self.ctx, C.c_uint32(0), None, None, None, None, None, *((convert.args(0) if convert else ()) + (vp,))))
            return verdicts
        ptrs = (C.POINTER(C.c_uint8) * count)()
        lens = (C.c_size_t * count)()
        if isinstance(proofs, ProofBatch):
            base = proofs._buf.ctypes.data
            for i in range(count):
                ptrs[i] = C.cast(C.c_void_p(base + i * proofs._stride), C.POINTER(C.c_uint8))
                lens[i] = int(proofs._lens[i])
            keep = proofs
        else:
            keep = [bytes(p) for p in proofs]
            for i, p in enumerate(keep):
                ptrs[i] = C.cast(C.c_char_p(p), C.POINTER(C.c_uint8))
                lens[i] = len(p)
        ir = np.ascontiguousarray(np.broadcast_to(np.asarray(initial_roots, np.uint64).reshape(-1, 7), (count, 7)))
        fr = np.ascontiguousarray(np.broadcast_to(np.asarray(final_roots, np.uint64).reshape(-1, 7), (count, 7)))
        o = None if options is None else C.byref(self._options_struct(options))
        if convert:
            convert.allocate(keep if isinstance(keep, list) else [bytes(p) for p in keep])
        check(fn(self.ctx, C.c_uint32(count), ptrs, lens, ir.ctypes.data_as(u64p), fr.ctypes.data_as(u64p), o,
                 *((convert.args(count) if convert else ()) + (vp,))))
        del keep
        return verdicts

    def air_verify(self, proofs, airs, public_inputs=None, options=None, numbers=None):
        """cstark_air_verify: proofs of TransactionAir, MerkleAir, RangeProofAir and RescueAir (bytes, any mix) in one call.  airs: the AIR
        each proof is expected to be (Backend.AIR_*; one value for all, or one per proof).  public_inputs: [count][14] words (or [14] for
        every proof), memory form -- initial root | final root, seed | result, or the range number in word 0.  numbers (instead of
        public_inputs, RangeProofAir only): one number for all proofs or [count] numbers.  options: as for tx_verify.  Returns the verdicts, int32 [count]; SchnorrAir proofs are UNSUPPORTED here (schnorr_verify takes their statement)."""
        return self._air_call(self.lib.cstark_air_verify, proofs, airs, public_inputs, options, numbers)

    def _air_call(self, fn, proofs, airs, public_inputs, options, numbers, convert=None):
        """cstark_air_verify, or cstark_air_convert with convert = _Conversion"""
        count = len(proofs)
        verdicts = np.zeros(count, np.int32)
        if count == 0:
            return verdicts
        keep = [bytes(p) for p in proofs]
        ptrs = (C.POINTER(C.c_uint8) * count)()
        lens = (C.c_size_t * count)()
        for i, p in enumerate(keep):
            ptrs[i] = C.cast(C.c_char_p(p), C.POINTER(C.c_uint8))
            lens[i] = len(p)
        ids = np.ascontiguousarray(np.broadcast_to(np.asarray(airs, np.int32).reshape(-1), (count,)))
        if (numbers is None) == (public_inputs is None):
            raise ValueError("give public_inputs ([count][14] or [14]) or numbers (RangeProofAir), not both")
        if numbers is not None:
            if (ids != self.AIR_RANGE).any():
                raise ValueError("numbers= states RangeProofAir proofs only")
            pub = np.zeros((count, 14), np.uint64)
            pub[:, 0] = np.broadcast_to(np.asarray(numbers, np.uint64).reshape(-1), (count,))
        else:
            pub = np.asarray(public_inputs, np.uint64)
            if pub.ndim not in (1, 2) or pub.shape[-1] != 14:
                raise ValueError("public_inputs must be [count][14] or [14]")
            pub = np.ascontiguousarray(np.broadcast_to(pub.reshape(-1, 14), (count, 14)))
        o = None if options is None else C.byref(self._options_struct(options))
        if convert:
            convert.allocate(keep)
        check(fn(self.ctx, C.c_uint32(count), ptrs, lens, ids.ctypes.data_as(C.POINTER(C.c_int32)), pub.ctypes.data_as(u64p), o,
                 *((convert.args(count) if convert else ()) + (verdicts.ctypes.data_as(C.POINTER(C.c_int32)),))))
        del keep
        return verdicts

    def schnorr_verify(self, proofs, statements, options=None):
        """cstark_schnorr_verify: SchnorrAir proofs (bytes) against their statements in one call.  statements: one (messages [n][28],
        sig_rx [n][6], sig_s [n][32]) triple per proof -- or an object with those attributes, such as a SchnorrExample -- memory form;
        the batch may mix numbers of signatures, hashes, extensions and options.  options: as for tx_verify.  Returns the verdicts, int32 [count]."""
        return self._schnorr_call(self.lib.cstark_schnorr_verify, proofs, statements, options)

    def _schnorr_call(self, fn, proofs, statements, options, convert=None):
        """cstark_schnorr_verify, or cstark_schnorr_convert with convert = _Conversion"""
        count = len(proofs)
        verdicts = np.zeros(count, np.int32)
        vp = verdicts.ctypes.data_as(C.POINTER(C.c_int32))
        if count == 0:
            check(fn(self.ctx, C.c_uint32(0), None, None, None, None, *((convert.args(0) if convert else ()) + (vp,))))
            return verdicts
        if len(statements) != count:
            raise ValueError("one statement per proof")
        keep = [bytes(p) for p in proofs]
        ptrs = (C.POINTER(C.c_uint8) * count)()
        lens = (C.c_size_t * count)()
        stm = (_lib.SchnorrStatementStruct * count)()
        arrays = []
        for i, (p, st) in enumerate(zip(keep, statements)):
            ptrs[i] = C.cast(C.c_char_p(p), C.POINTER(C.c_uint8))
            lens[i] = len(p)
            msg, rx, s = (st.messages, st.sig_rx, st.sig_s) if hasattr(st, "messages") else st
            msg = np.ascontiguousarray(np.asarray(msg, np.uint64).reshape(-1, 28))
            rx = np.ascontiguousarray(np.asarray(rx, np.uint64).reshape(-1, 6))
            s = np.ascontiguousarray(np.asarray(s, np.uint8).reshape(-1, 32))
            if not (msg.shape[0] == rx.shape[0] == s.shape[0]):
                raise ValueError("messages, sig_rx and sig_s state different numbers of signatures")
            arrays.append((msg, rx, s))
            stm[i].n_sig = msg.shape[0]
            stm[i].messages, stm[i].sig_rx, stm[i].sig_s = msg.ctypes.data_as(u64p), rx.ctypes.data_as(u64p), s.ctypes.data_as(_lib.u8p)
        o = None if options is None else C.byref(self._options_struct(options))
        if convert:
            convert.allocate(keep)
        check(fn(self.ctx, C.c_uint32(count), ptrs, lens, stm, o, *((convert.args(count) if convert else ()) + (vp,))))
        del keep, arrays
        return verdicts

    # ---- conversion between the proof forms (cstark_tx_convert, cstark_air_convert, cstark_schnorr_convert) -----------------------
    def tx_convert(self, proofs, initial_roots, final_roots, form, options=None):
        """cstark_tx_convert: tx_verify that also writes every accepted proof in `form` ("plain" or "compact"), byte for byte what the
        prover writes in that form; a proof already in it comes back unchanged.  Returns (converted, verdicts): converted[i] is the bytes,
        or None where verdicts[i] is not OK; the verdicts are tx_verify's for the same arguments.  The prover's state and proof_form are
        not touched."""
        cv = _Conversion(self, form)
        verdicts = self._tx_call(self.lib.cstark_tx_convert, proofs, initial_roots, final_roots, options, cv)
        return cv.results(verdicts), verdicts

    def air_convert(self, proofs, airs, public_inputs=None, form=None, options=None, numbers=None):
        """cstark_air_convert: air_verify that also writes every accepted proof in `form`; returns (converted, verdicts) as tx_convert.  A
        SchnorrAir proof is UNSUPPORTED here and not converted (schnorr_convert)."""
        cv = _Conversion(self, form)
        verdicts = self._air_call(self.lib.cstark_air_convert, proofs, airs, public_inputs, options, numbers, cv)
        return cv.results(verdicts), verdicts

    def schnorr_convert(self, proofs, statements, form, options=None):
        """cstark_schnorr_convert: schnorr_verify that also writes every accepted proof in `form`; returns (converted, verdicts)"""
        cv = _Conversion(self, form)
        verdicts = self._schnorr_call(self.lib.cstark_schnorr_convert, proofs, statements, options, cv)
        return cv.results(verdicts), verdicts

    def schnorr_public_at(self, messages, sig_rx, z):
        """cstark_schnorr_public_at: the 19 public-input columns and the 12 sequence-value polynomials of the statement at z (m words,
        memory form, m = 1, 2 or 3) -> uint64 [31][m]"""
        msg = np.ascontiguousarray(np.asarray(messages, np.uint64).reshape(-1, 28))
        rx = np.ascontiguousarray(np.asarray(sig_rx, np.uint64).reshape(-1, 6))
        if msg.shape[0] != rx.shape[0]:
            raise ValueError("messages and sig_rx state different numbers of signatures")
        zz = np.ascontiguousarray(np.asarray(z, np.uint64).reshape(-1))
        out = np.zeros((31, zz.size), np.uint64)
        check(self.lib.cstark_schnorr_public_at(self.ctx, C.c_uint32(msg.shape[0]), msg.ctypes.data_as(u64p), rx.ctypes.data_as(u64p),
                                                zz.ctypes.data_as(u64p), C.c_uint32(zz.size), out.ctypes.data_as(u64p)))
        return out

    def verify_h2d_bytes(self):
        """bytes the last tx_verify / air_verify / schnorr_verify copied host -> device: proof bytes, descriptors and opening records"""
        n = C.c_uint64(0)
        check(self.lib.cstark_verify_h2d_bytes(self.ctx, C.byref(n)))
        return int(n.value)

    def verify_stage_ms(self):
        from .verify import VERIFY_STAGES
        ms = (C.c_float * len(VERIFY_STAGES))()
        check(self.lib.cstark_verify_stage_ms(self.ctx, ms))
        return dict(zip(VERIFY_STAGES, [float(v) for v in ms]))

    def air_prove(self, air, options, number=0):
        """cstark_air_prove: complete proof of the uploaded witness under MerkleAir / SchnorrAir, or of `number` (memory form)
        under RangeProofAir."""
        o = _lib.OptionsStruct(options.num_queries, options.blowup_factor, options.grinding_factor, options.hash_fn,
                               options.field_extension, options.fri_folding_factor, options.fri_max_remainder)
        self.lib.cstark_tx_proof_size_bound.restype = C.c_size_t
        cap = 2 * self.lib.cstark_tx_proof_size_bound(C.c_uint32(max(1, self.n_tx)), C.byref(o))
        buf = (C.c_uint8 * cap)()
        n = C.c_size_t(0)
        check(self.lib.cstark_air_prove(self.ctx, C.c_int(air), C.byref(o), C.c_uint64(number), buf, C.c_size_t(cap), C.byref(n)))
        return bytes(memoryview(buf)[:n.value])
