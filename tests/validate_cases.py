"""Reference for trace validation -- shared by test_validate_reference_cpu.py (CPU) and test_gpu_validate.py / test_gpu_cpp_validate.py.

What cstark_air_validate_trace must report, from the CPU oracle alone: the transition-constraint values of every frame (r, r + 1),
r < n - 1, of a base trace (oracle.air_evaluate_transitions / oracle.schnorr_evaluate_transitions at blowup 1 with the RAW periodic
columns, the _check_trace pattern of test_oracle_small_airs.py; per-row oracle.tx_evaluate_transition for TransactionAir), reduced to
per-cycle codes, the first violation and the boundary verdict over the AirDesc assertion lists.  Not a conftest."""
import numpy as np

from cheating_prover import CELLS

P = (1 << 62) + (1 << 56) + (1 << 55) + 1
CLEAN = 0xFFFFFFFF
TX, MERKLE, SCHNORR, RANGE, RESCUE = 0, 1, 2, 3, 4
NC = {TX: 115, MERKLE: 106, SCHNORR: 56, RANGE: 2, RESCUE: 14}
WIDTH = {TX: 94, MERKLE: 65, SCHNORR: 56, RANGE: 2, RESCUE: 14}
CYCLE = {TX: 1024, MERKLE: 512, SCHNORR: 512, RANGE: 0, RESCUE: 8}   # 0: the whole trace is one cycle

# (column, row) of a two-transfer TransactionAir trace (2048 rows); shared with the GPU tests
TX_CELLS = dict(CELLS)
TX_CELLS.update({
    "row-0": (3, 0), "last-row": (60, 2047), "row-n-2": (70, 2046), "row-1023": (60, 1023), "row-1024": (60, 1024),
    "row-63": (61, 63), "row-64": (61, 64), "slot-0": (0, 600), "top-slot": (88, 300),
    "prev-root-finish": (58, 511), "prev-root-not-finish": (58, 100),
})


def one():
    from oracle import oracle as O
    return int(O.to_mont([1])[0])


def bump(trace, cells):
    """a copy of the trace with 1 (memory form) added mod p to every (column, row) of `cells`"""
    t = np.array(trace, np.uint64, copy=True)
    for c, r in cells:
        t[c, r] = np.uint64((int(t[c, r]) + one()) % P)
    return t


class Reference:
    """per-cycle codes, first violation, values of the first violated frame: from the constraint values ev [nc][n - 1]"""

    def __init__(self, air, ev):
        nc, m = ev.shape
        assert nc == NC[air]
        n = m + 1
        cyc = CYCLE[air] or n
        self.codes = np.full(n // cyc, CLEAN, np.uint32)
        bad = ev != 0
        rows = np.nonzero(bad.any(axis=0))[0]
        for r in rows:                                   # ascending: the first violated row of a cycle, its lowest violated slot
            if self.codes[r // cyc] == CLEAN:
                self.codes[r // cyc] = (r % cyc) * nc + int(np.argmax(bad[:, r]))
        self.bad_cycles = int((self.codes != CLEAN).sum())
        self.step = int(rows[0]) if rows.size else None
        self.constraint = int(np.argmax(bad[:, rows[0]])) if rows.size else None
        self.frame_values = ev[:, rows[0]].copy() if rows.size else None


def sub_air_values(O, air, trace, depth=0, statement=None):
    """ev [nc][n - 1] of MerkleAir, SchnorrAir (statement: a SchnorrWitness), RangeProofAir or RescueAir on the base trace"""
    width, n = trace.shape
    lde = np.ascontiguousarray(trace).reshape(1, width, n)
    if air == SCHNORR:
        aux = O.schnorr_aux_columns(statement).reshape(1, 19, n)
        ev = O.schnorr_evaluate_transitions(lde, aux, O.schnorr_mask_columns().reshape(1, 36, 512))[0]
    else:
        cols = {MERKLE: lambda: O.merkle_periodic_columns(depth), RESCUE: O.rescue_chain_periodic_columns, RANGE: lambda: None}[air]()
        ptab = None if cols is None else cols.reshape(1, cols.shape[0], cols.shape[1])
        ev = O.air_evaluate_transitions(air, lde, ptab, NC[air])[0]
    return ev[:, :n - 1]


def tx_values(O, trace, depth, rows=None):
    """ev [115][n - 1] of TransactionAir, row by row (oracle.tx_evaluate_transition); rows: only these frames (the others read 0)"""
    n = trace.shape[1]
    per = O.tx_periodic_columns(depth)
    ev = np.zeros((115, n - 1), np.uint64)
    tr = np.ascontiguousarray(trace.T)
    for r in (range(n - 1) if rows is None else rows):
        ev[:, r] = O.tx_evaluate_transition(tr[r], tr[r + 1], np.ascontiguousarray(per[:, r % 1024]))
    return ev


def tx_reference(O, trace, clean_trace, depth):
    """Reference of a TransactionAir trace that differs from a trace KNOWN to be clean (every frame evaluated once, in
    test_validate_reference_cpu.py) in a few cells: a frame's values depend on rows r and r + 1 alone, so only the frames next to a
    changed row are evaluated again."""
    n = trace.shape[1]
    changed = np.nonzero((trace != clean_trace).any(axis=0))[0]
    rows = sorted({int(r) + d for r in changed for d in (-1, 0) if 0 <= int(r) + d < n - 1})
    return Reference(TX, tx_values(O, trace, depth, rows))


def reference(O, air, trace, depth=0, statement=None, clean_trace=None):
    if air == TX:
        return tx_reference(O, trace, clean_trace, depth) if clean_trace is not None else Reference(TX, tx_values(O, trace, depth))
    return Reference(air, sub_air_values(O, air, trace, depth, statement))


def boundary_list(O, air, n, public=None, statement=None):
    """[(register, [steps], [values])] in the order of cstark_trace_report::boundary, from the AirDesc assertion lists"""
    if air in (TX, MERKLE, RESCUE):
        r0 = 0 if air == RESCUE else 58
        return [(r0 + a % 7, [0 if a < 7 else n - 1], [int(public[a])]) for a in range(14)]
    if air == RANGE:
        return [(1, [0], [0]), (1, [n - 1], [int(public[0])])]
    d = O.schnorr_desc(statement)
    out = []
    for a in range(d.na):
        steps = list(range(int(d.a_first[a]), n, int(d.a_stride[a])))
        q = int(d.a_seq[a])
        vals = [int(statement.sig_rx[t, q % 6]) for t in range(len(steps))] if q >= 0 else [int(d.a_value[a])] * len(steps)
        out.append((int(d.a_reg[a]), steps, vals))
    return out


def boundary_reference(O, air, trace, public=None, statement=None):
    """(entry, register, step) of the first failing entry and its lowest failing step, or None"""
    for k, (reg, steps, vals) in enumerate(boundary_list(O, air, trace.shape[1], public, statement)):
        for s, v in zip(steps, vals):
            if int(trace[reg, s]) != v:
                return k, reg, s
    return None
