"""A plain model of Ledger.select (cstark_ledger_select) over the ledger model (ledger_model.py): the rule of include/cstark.h stated as
one sequential loop in Python integers.  Candidates are examined in list order, each against the accounts as the candidates selected
before it leave them, and a candidate gets the first status that applies:

    NOT_REACHED (9)   `want` candidates are selected already
    INDEX_RANGE (1), SELF_TRANSFER (2), UNKNOWN (6, a partial ledger only), ABSENT (3)
    HELD (8)          an earlier candidate of this call with the same sender index was refused, with any status but NOT_REACHED
    BALANCE (4)       delta above the sender's balance, both as canonical integers
    SIGNATURE (5)     only with a sig_ok callable: a sig_rx word >= p, or sig_ok(t, message) is false
    APPLIED (0)       selected: balances move and the sender's nonce counts up

A refused candidate whose sender index is in range holds that sender for the rest of the call; a held account still receives.  The
model keeps every account's nonce as the selected candidates leave it and builds each message from that state: it knows nothing of the
product's shortcut (the stored nonce plus the number of earlier candidates of the sender), which the hold makes valid.  pow2 is stated
as the issue states it: the same call again with `want` = the largest power of two not above the number selected."""
import numpy as np

import ledger_model as LM

P = LM.P
APPLIED, INDEX_RANGE, SELF_TRANSFER, ABSENT, BALANCE, SIGNATURE, UNKNOWN, KEY, HELD, NOT_REACHED = range(10)


class Result:
    def __init__(self, status, selected, messages):
        self.status = np.array(status, np.uint8)
        self.selected = np.array(selected, np.uint32)
        self.messages = messages          # candidate number -> uint64 [28], for every candidate that reached the signature test

    @property
    def counts(self):
        return [int((self.status == k).sum()) for k in range(10)]

    def transfers(self, pool):
        """the arrays of the selection, what LedgerModel.apply and Ledger.apply take"""
        return tuple(np.asarray(a)[self.selected] for a in pool)


def select(model, s, r, deltas, want, sig_ok=None, sig_rx=None, pow2=False, known=None):
    """model: a LedgerModel (read only).  deltas in memory form.  sig_ok: None (signatures are not checked) or a callable
    (t, message uint64 [28]) -> bool, asked only about candidates that reach the signature test with a reduced sig_rx (sig_rx: [n][6]
    or None).  known: the leaves a partial ledger knows (None: a full ledger)."""
    res = _select(model, s, r, deltas, want, sig_ok, sig_rx, known)
    if pow2 and len(res.selected):
        keep = 1 << (len(res.selected).bit_length() - 1)
        res = _select(model, s, r, deltas, keep, sig_ok, sig_rx, known)
    return res


def _select(model, s, r, deltas, want, sig_ok, sig_rx, known):
    n, size = len(s), 1 << model.depth
    balance = {a: LM.canonical(v[12]) for a, v in model.value.items()}
    nonce = {a: LM.canonical(v[13]) for a, v in model.value.items()}
    held, status, selected, messages = set(), [], [], {}
    for t in range(n):
        si, ri, delta = int(s[t]), int(r[t]), LM.canonical(deltas[t])
        if len(selected) == want:
            status.append(NOT_REACHED)
            continue
        if si >= size or ri >= size:
            st = INDEX_RANGE
        elif si == ri:
            st = SELF_TRANSFER
        elif known is not None and (si not in known or ri not in known):
            st = UNKNOWN
        elif si not in model.value or ri not in model.value:
            st = ABSENT
        elif si in held:
            st = HELD
        elif delta > balance[si]:
            st = BALANCE
        else:
            st = APPLIED
            if sig_ok is not None:
                m = np.zeros(28, np.uint64)
                m[0:12], m[12:24], m[24], m[25] = model.value[si][:12], model.value[ri][:12], deltas[t], LM.memory(nonce[si])
                messages[t] = m
                if sig_rx is not None and any(int(w) >= P for w in sig_rx[t]):
                    st = SIGNATURE
                elif not sig_ok(t, m):
                    st = SIGNATURE
        status.append(st)
        if st != APPLIED:
            if si < size:
                held.add(si)
            continue
        balance[si] = (balance[si] - delta) % P
        balance[ri] = (balance[ri] + delta) % P
        nonce[si] = (nonce[si] + 1) % P
        selected.append(t)
    return Result(status, selected, messages)
