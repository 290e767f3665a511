"""Python references for the compact proof form (include/cstark.h, "Proof layout"): no GPU, no library code.

A compact proof ("CSTC") is the plain proof ("CSTK") with each of its 2 + n_layers path sections replaced by `u32 n_nodes |
nodes[n_nodes][32]`, the Merkle multiproof of that tree for the sorted distinct positions opened in it.  Positions are not stored in
either form; here they come from the `probe` of the CPU verifier (oracle.verifier.verify / verify_range).

    multiproof_nodes(depth, positions)    the (level, index) of the multiproof's nodes, in the canonical order
    compact(plain, positions)             plain bytes -> compact bytes, by selection from the per-query paths
    expand(compact, positions, hash_fn)   compact bytes -> plain bytes: every path rebuilt from rows, nodes and computed parents
    walk(proof)                           the sections of a proof of either form (offsets for the tampering tests)

The shared inputs (CPU proofs and their positions) are computed once per process and never changed."""
import struct

import numpy as np

SHAPES = {0: (94, 8), 1: (65, 4), 2: (56, 8), 3: (2, 2), 4: (14, 4)}  # air id -> (trace width, composition columns)

# TransactionAir: witness(2, 3) at these options; RangeProofAir: the number 42 at these
TX_OPTS = [(42, 8, 0, 0, 0, 4, 256), (42, 8, 0, 1, 0, 4, 256), (20, 16, 0, 0, 2, 16, 128), (20, 8, 0, 0, 1, 8, 128)]
RANGE_OPTS = [(42, 4, 0, 0, 0, 4, 256), (42, 8, 0, 0, 0, 4, 128), (64, 2, 0, 0, 0, 4, 128), (128, 4, 0, 1, 2, 4, 128), (128, 16, 0, 0, 1, 16, 128)]


def multiproof_nodes(depth, positions):
    """K_depth = the distinct positions; for l = depth .. 1 every x of K_l, ascending, contributes (l, x ^ 1) iff x ^ 1 is not in K_l;
    K_(l-1) = the parents"""
    level, nodes = sorted(set(positions)), []
    for l in range(depth, 0, -1):
        have = set(level)
        nodes += [(l, x ^ 1) for x in level if x ^ 1 not in have]
        level = sorted({x >> 1 for x in level})
    return nodes


class Tree:
    """one tree's sections inside a proof: rows at `rows` (count of them, row_bytes each), then the path section: plain -> paths at
    `paths` [count][depth][32]; compact -> the count word at `paths - 4`, n_nodes nodes at `paths`"""

    def __init__(self, name, rows, count, row_bytes, depth):
        self.name, self.rows, self.count, self.row_bytes, self.depth = name, rows, count, row_bytes, depth
        self.paths, self.n_nodes, self.end = None, None, None


def walk(proof):
    """-> (form, [Tree...] in proof order: trace, composition, layer 0 ..., offset of the remainder's count word).  Reads the counts the
    proof states; raises ValueError when they run past the end."""
    b = bytes(proof)
    form = {b"CSTK": "plain", b"CSTC": "compact"}[b[:4]]
    air, width, log_n, _ = struct.unpack_from("<4I", b, 8)
    nq, blowup, _, _, ext, folding, _ = struct.unpack_from("<7I", b, 24)
    ce, em = SHAPES[air][1], ext + 1
    log_N, log_f = log_n + blowup.bit_length() - 1, folding.bit_length() - 1
    nl = struct.unpack_from("<I", b, 116)[0]
    o = 120 + 32 * nl + 32 + 8 * (2 * width + ce) * em + 8
    trees = []

    def tree(name, o, count, row_bytes, depth):
        t = Tree(name, o, count, row_bytes, depth)
        o += count * row_bytes
        if form == "plain":
            t.paths, t.n_nodes = o, count * depth
        else:
            t.n_nodes = struct.unpack_from("<I", b, o)[0]
            t.paths = o + 4
        t.end = t.paths + 32 * t.n_nodes
        if t.end > len(b):
            raise ValueError("sections run past the end")
        trees.append(t)
        return t.end

    o = tree("trace", o, nq, 8 * width, log_N)
    o = tree("composition", o, nq, 8 * ce * em, log_N)
    lg = log_N
    for l in range(nl):
        npos = struct.unpack_from("<I", b, o)[0]
        lg -= log_f
        o = tree("layer%d" % l, o + 4, npos, 8 * folding * em, lg)
    return form, trees, o


def tree_positions(proof, positions):
    """the positions opened in every tree, in proof order (one list per Tree of walk): the query positions twice, then every layer's
    folded positions"""
    from oracle import verifier as V
    _, trees, _ = walk(proof)
    out, cur = [list(positions), list(positions)], list(positions)
    for t in trees[2:]:
        cur = V.fold_positions(cur, 1 << t.depth)
        out.append(cur)
    return out


def compact(plain, positions):
    b = bytes(plain)
    form, trees, _ = walk(b)
    assert form == "plain"
    out, o = bytearray(b"CSTC"), 4
    for t, pos in zip(trees, tree_positions(b, positions)):
        assert len(pos) == t.count
        out += b[o:t.paths]
        nodes = []
        for l, y in multiproof_nodes(t.depth, pos):
            q = next(q for q, p in enumerate(pos) if p >> (t.depth - l) == y ^ 1)     # any query below the node's sibling
            at = t.paths + 32 * (q * t.depth + t.depth - l)
            nodes.append(b[at:at + 32])
        out += struct.pack("<I", len(nodes)) + b"".join(nodes)
        o = t.end
    return bytes(out + b[o:])


def expand(compact_bytes, positions, hash_fn):
    """hash_fn: the proof's hash id (0 Blake3, 1 Sha3).  Raises ValueError when a tree's node count is not the multiproof's."""
    from oracle import oracle as O
    from oracle import verifier as V
    b = bytes(compact_bytes)
    form, trees, _ = walk(b)
    assert form == "compact"
    out, o = bytearray(b"CSTK"), 4
    for t, pos in zip(trees, tree_positions(b, positions)):
        assert len(pos) == t.count
        out += b[o:t.paths - 4]
        want = multiproof_nodes(t.depth, pos)
        if len(want) != t.n_nodes:
            raise ValueError("%s: %d nodes stated, the positions ask for %d" % (t.name, t.n_nodes, len(want)))
        known = {node: b[t.paths + 32 * i:t.paths + 32 * i + 32] for i, node in enumerate(want)}
        for q, p in enumerate(pos):
            row = np.frombuffer(b[t.rows + q * t.row_bytes:t.rows + (q + 1) * t.row_bytes], np.uint64)
            known[(t.depth, p)] = O.digest(V.elem_bytes(row), hash_fn)
        level = sorted(set(pos))
        for l in range(t.depth, 0, -1):
            for x in level:
                known[(l - 1, x >> 1)] = O.digest(known[(l, x & ~1)] + known[(l, x | 1)], hash_fn)
            level = sorted({x >> 1 for x in level})
        for p in pos:
            out += b"".join(known[(t.depth - j, (p >> j) ^ 1)] for j in range(t.depth))
        o = t.end
    return bytes(out + b[o:])


# ---- the shared inputs -------------------------------------------------------------------------------------------------------------
_witnesses, _cases = {}, {}


def witness(n_tx, depth):
    from oracle import oracle as O
    if (n_tx, depth) not in _witnesses:
        _witnesses[(n_tx, depth)] = O.TxWitness.generate(n_tx, depth, seed=900 + n_tx)
    return _witnesses[(n_tx, depth)]


def range_number(value=42):
    from oracle import oracle as O
    return int(O.to_mont([value])[0])


def tx_case(n_tx, depth, opts):
    """-> (the CPU prover's plain proof, the query positions the CPU verifier derived from it)"""
    from oracle import prover as OP
    from oracle import verifier as V
    key = ("tx", n_tx, depth, tuple(opts))
    if key not in _cases:
        w = witness(n_tx, depth)
        proof, probe = OP.prove(w, tuple(opts)), {}
        assert V.verify(proof, w.initial_roots[0], w.final_root, options=list(opts), probe=probe)
        _cases[key] = (proof, probe["positions"])
    return _cases[key]


def range_case(opts, value=42):
    from oracle import oracle as O
    from oracle import prover as OP
    from oracle import verifier as V
    key = ("range", tuple(opts), value)
    if key not in _cases:
        proof, probe = OP.prove_air(O.AIR_RANGE, range_number(value), tuple(opts)), {}
        assert V.verify_range(proof, range_number(value), options=list(opts), probe=probe)
        _cases[key] = (proof, probe["positions"])
    return _cases[key]


def outside_paths(proof):
    """the bytes of a proof of either form without its magic and its path sections (a compact section: the count word and the nodes)"""
    b = bytes(proof)
    form, trees, _ = walk(b)
    out, o = b"", 4
    for t in trees:
        out += b[o:t.paths - (4 if form == "compact" else 0)]
        o = t.end
    return out + b[o:]


def path_digests(proof):
    """the number of digests in the path sections of a proof of either form"""
    return sum(t.n_nodes for t in walk(proof)[1])
