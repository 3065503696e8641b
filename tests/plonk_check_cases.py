"""Shared by tests/test_plonk_check_host.py and tests/test_gpu_plonk_check.py (not a test module): a model of "the witness satisfies the circuit" in plain
Python integers -- the definition of include/bbgpu.h (bbgpu_plonk_check_witness), written down once more, independent of the library -- the fixture
circuits, and the list of perturbed witnesses / circuits each of them is tried with.  The targets of the perturbations are chosen WITH the model
(a changed wire of a padding row breaks nothing; in the extended fixture a changed w_o of row n/4 breaks copy constraints and no gate)."""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R_MOD = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001
RINV = pow(1 << 256, -1, R_MOD)
NONE = 0xFFFFFFFF
ARITH, BOOL_L, BOOL_R, BOOL_O, MIMC_CUBE, MIMC_OUT = 1, 2, 4, 8, 16, 32
WIRES = ("w_l", "w_r", "w_o")
MAPS = ("sigma_1_mapping", "sigma_2_mapping", "sigma_3_mapping")
MIMC_X0 = 0x0777777788888888555555556666666633333333444444441111111122222222  # tests/test_gpu_plonk.py
MIMC_K = 0x0ABCDEFABCDEFABC1234123412341234DDDDEEEEFFFF00009999AAAABBBBCCCC
A0 = 0x0777777788888888555555556666666633333333444444441111111122222222
B0 = 0x0ABCDEFABCDEFABC1234123412341234DDDDEEEEFFFF00009999AAAABBBBCCCC
FIELDS = ("gate_failures", "copy_failures", "first_gate", "first_gate_kinds", "kinds", "first_copy", "first_copy_target")
CLEAR = {"gate_failures": 0, "copy_failures": 0, "first_gate": NONE, "first_gate_kinds": 0, "kinds": 0, "first_copy": NONE, "first_copy_target": NONE}


def raw_ints(a):
    """(n, 4) uint64 -> the 256-bit integers as they stand in memory (any representative)"""
    o = np.asarray(a, dtype=np.uint64).astype(object)
    return (o[:, 0] + (o[:, 1] << 64) + (o[:, 2] << 128) + (o[:, 3] << 192)).tolist()


def limbs(v):
    return np.array([(v >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for k in range(4)], dtype=np.uint64)


def mont(v):
    return limbs((v << 256) % R_MOD)


class Model:
    """the yardstick: rows 0 .. n-2, every identity on its own, copy constraints with the prover's decoding of the mapping entries"""

    def __init__(self, state):
        self.n = int(state["n"])
        self.rows = self.n - 1
        self.w = [[v * RINV % R_MOD for v in raw_ints(state[k])] for k in WIRES]
        self.q = {k: [v * RINV % R_MOD for v in raw_ints(state[k])] for k in state if k.startswith("q_")}
        self.maps = [[int(m) for m in state[k]] for k in MAPS]

    def clone(self):
        c = Model.__new__(Model)
        c.n, c.rows, c.q = self.n, self.rows, self.q
        c.w = [list(v) for v in self.w]
        c.maps = [list(m) for m in self.maps]
        return c

    def kinds_present(self):
        """the identity kinds a witness CAN fail in this circuit: a widget's identity whose selector is zero in every constrained row holds for every
        witness (the bool fixture circuit constrains no output wire: its q_bo is zero throughout)"""
        def live(sel):
            return sel in self.q and any(self.q[sel][:self.rows])
        k = ARITH
        for bit, sel in ((BOOL_L, "q_bl"), (BOOL_R, "q_br"), (BOOL_O, "q_bo"), (MIMC_CUBE, "q_mimc_selector"), (MIMC_OUT, "q_mimc_selector")):
            if live(sel):
                k |= bit
        return k

    def gate_kinds(self, i):
        q, (wl, wr, wo) = self.q, (self.w[0][i], self.w[1][i], self.w[2][i])
        k = 0
        a = q["q_m"][i] * wl * wr + q["q_l"][i] * wl + q["q_r"][i] * wr + q["q_o"][i] * wo + q["q_c"][i]
        if "q_o_next" in q:
            a += q["q_o_next"][i] * self.w[2][i + 1]
        if a % R_MOD:
            k |= ARITH
        if "q_bl" in q:
            for bit, sel, w in ((BOOL_L, "q_bl", wl), (BOOL_R, "q_br", wr), (BOOL_O, "q_bo", wo)):
                if q[sel][i] * (w * w - w) % R_MOD:
                    k |= bit
        if "q_mimc_selector" in q:
            t = wo + wl + q["q_mimc_coefficient"][i]
            if q["q_mimc_selector"][i] * (t * t * t - wr) % R_MOD:
                k |= MIMC_CUBE
            if q["q_mimc_selector"][i] * (t * wr * wr - self.w[2][i + 1]) % R_MOD:
                k |= MIMC_OUT
        return k

    def target(self, m):
        """(row, wire) of a mapping entry, as k_sigma_from_mapping decodes it: code 3 reads as the left wire"""
        t = (m >> 30) & 3
        return (m & ((1 << 29) - 1)) & (self.n - 1), 0 if t == 3 else t

    def copy_ok(self, i, k):
        row, wire = self.target(self.maps[k][i])
        return row < self.rows and self.w[wire][row] == self.w[k][i]

    def report(self):
        r = dict(CLEAR)
        for i in range(self.rows):
            k = self.gate_kinds(i)
            if k:
                if r["first_gate"] == NONE:
                    r["first_gate"], r["first_gate_kinds"] = i, k
                r["kinds"] |= k
                r["gate_failures"] += 1
            for wire in range(3):
                if not self.copy_ok(i, wire):
                    if r["first_copy"] == NONE:
                        r["first_copy"], r["first_copy_target"] = i | (wire << 30), self.maps[wire][i]
                    r["copy_failures"] += 1
        return r


def is_clear(rep):
    return rep["gate_failures"] == 0 and rep["copy_failures"] == 0


# ---- circuits ----------------------------------------------------------------------------------------------------------------------------------------
def add_chain_circuit(gates):
    """a StandardComposer circuit of exactly `gates` add gates c = a + b, chained: with gates = 2^k - 1 row n-2 holds the last real gate"""
    from barretenberg_amd.plonk import StandardComposer
    c = StandardComposer()
    a, b = 3, 5
    ai, bi = c.add_variable(a), c.add_variable(b)
    for _ in range(gates):
        s = (a + b) % R_MOD
        si = c.add_variable(s)
        c.create_add_gate(ai, bi, si, 1, 1, -1, 0)
        a, ai, b, bi = b, bi, s, si
    return c


def extended_state(gates):
    z = np.load(os.path.join(ROOT, "tests", "golden", "plonk_extended_state.npz"))
    st = {k.split("/", 1)[1]: z[k] for k in z.files if k.startswith("%d/" % gates)}
    st["n"] = int(st["n"][0])
    return st


def circuit(name):
    from barretenberg_amd.plonk import bench_circuit, bool_circuit, mimc_circuit
    kind, size = name.split("_")
    size = int(size)
    if kind == "bench":
        return bench_circuit(size, A0, B0).preprocess()
    if kind == "bool":
        return bool_circuit(size).preprocess()
    if kind == "mimc":
        return mimc_circuit(size, MIMC_X0, MIMC_K).preprocess()
    if kind == "ext":
        return extended_state(size)
    if kind == "addchain":
        return add_chain_circuit(size).preprocess()
    raise KeyError(name)


FIXTURES = ("bench_64", "bench_4096", "bool_64", "bool_4096", "mimc_93", "mimc_4094", "ext_100", "ext_160")
LAST_ROW_REAL = ("addchain_63", "addchain_1023", "mimc_63")  # row n-2 holds a real gate
ALL_CIRCUITS = FIXTURES + LAST_ROW_REAL


# ---- perturbations -------------------------------------------------------------------------------------------------------------------------------------
class Case:
    def __init__(self, name, state, circuit_changed=False, covers=()):
        self.name, self.state, self.circuit_changed, self.covers = name, state, circuit_changed, tuple(covers)

    def witness(self):
        return tuple(self.state[k] for k in WIRES)


def with_wires(state, changes):
    """changes: (wire, row, plain value) -> a state with those wire values replaced (canonical Montgomery limbs)"""
    st = dict(state)
    for wire, row, value in changes:
        k = WIRES[wire]
        if st[k] is state[k]:
            st[k] = np.array(state[k], dtype=np.uint64, copy=True)
        st[k][row] = mont(value % R_MOD)
    return st


def with_mapping(state, wire, row, entry):
    st = dict(state)
    st[MAPS[wire]] = np.array(state[MAPS[wire]], dtype=np.uint32, copy=True)
    st[MAPS[wire]][row] = np.uint32(entry)
    return st


def other_representatives(state):
    """every wire value v replaced by v + 2r, or v + r, whichever still lies below 2^256 (v + r always does for a canonical v < r < 2^254)"""
    st = dict(state)
    for k in WIRES:
        out = np.empty_like(np.asarray(state[k], dtype=np.uint64))
        for i, v in enumerate(raw_ints(state[k])):
            v %= R_MOD
            cand = v + (2 * R_MOD if i % 2 == 0 else R_MOD)
            assert cand < (1 << 256)
            out[i] = limbs(cand)
        st[k] = out
    return st


def _search(model, rows, want):
    """first (row, wire) in `rows` whose wire value + 1 makes `want(clone, row)` true"""
    for row in rows:
        for wire in (2, 0, 1):
            c = model.clone()
            c.w[wire][row] = (c.w[wire][row] + 1) % R_MOD
            if want(c, row):
                return row, wire
    return None


def cases(name, state):
    """-> [Case]: the honest witness first, then the fixed list of perturbations that apply to this circuit"""
    M = Model(state)
    n, rows = M.n, M.rows
    out = [Case("honest", state)]
    real = [i for i in range(rows) if any(M.q[k][i] for k in M.q)]  # rows with a non-zero selector
    assert real
    bump = lambda wire, row: (wire, row, M.w[wire][row] + 1)  # noqa: E731

    # one wire value of a middle row: ARITH there (and the copy constraints of its cycle)
    later = [r for r in real if r >= real[len(real) // 2]]
    mid = _search(M, later, lambda c, r: c.gate_kinds(r) & ARITH) or _search(M, later, lambda c, r: c.gate_kinds(r))  # (a MiMC chain has one arithmetic gate)
    assert mid is not None
    out.append(Case("middle_row", with_wires(state, [bump(mid[1], mid[0])]), covers=("ARITH",)))
    # row 0
    out.append(Case("row_0", with_wires(state, [bump(0, 0)])))
    # the last constrained row, n-2 (a real gate only in LAST_ROW_REAL: elsewhere free padding, where the model rightly reports nothing)
    out.append(Case("row_n-2", with_wires(state, [bump(2, n - 2)])))
    # row n-1 only: not constrained
    out.append(Case("row_n-1_only", with_wires(state, [(0, n - 1, 7), (1, n - 1, 9), (2, n - 1, 11)])))
    # other representatives of the same residues
    out.append(Case("representatives", other_representatives(state)))
    # two failing rows far apart
    lo = _search(M, real[len(real) // 8:], lambda c, r: c.gate_kinds(r) and not (r and c.gate_kinds(r - 1)))
    if lo is not None:
        def two(c, r):
            c.w[lo[1]][lo[0]] = (M.w[lo[1]][lo[0]] + 1) % R_MOD
            return r > lo[0] + 2 and c.gate_kinds(r) and c.report()["gate_failures"] == 2
        hi = _search(M, real[::-1][:16], two)
        if hi is not None:
            out.append(Case("two_rows", with_wires(state, [bump(lo[1], lo[0]), bump(hi[1], hi[0])])))
    # bool widget: a constrained wire set to 2
    for bit, sel, wire, label in ((BOOL_L, "q_bl", 0, "BOOL_L"), (BOOL_R, "q_br", 1, "BOOL_R"), (BOOL_O, "q_bo", 2, "BOOL_O")):
        if sel in M.q:
            at = [i for i in real[len(real) // 3:] + real[:len(real) // 3] if M.q[sel][i]]
            if at:
                out.append(Case("bool_2_" + label, with_wires(state, [(wire, at[0], 2)]), covers=(label,)))
    # MiMC widget: w_r of a MiMC gate (both MiMC identities)
    if "q_mimc_selector" in M.q:
        at = [i for i in real[len(real) // 3:] if M.q["q_mimc_selector"][i]][0]
        out.append(Case("mimc_w_r", with_wires(state, [bump(1, at)]), covers=("MIMC_CUBE", "MIMC_OUT")))
    # sequential widget: the successor's output wire of a row with q_o_next != 0 (the row's own three wires stay as they are)
    if "q_o_next" in M.q:
        at = [i for i in real[len(real) // 3:] if M.q["q_o_next"][i] and i + 1 < rows][0]
        c = M.clone()
        c.w[2][at + 1] = (c.w[2][at + 1] + 1) % R_MOD
        assert c.gate_kinds(at) & ARITH
        out.append(Case("seq_successor", with_wires(state, [bump(2, at + 1)]), covers=("Q_O_NEXT",)))
    # one mapping entry redirected (these change the CIRCUIT): to an equal value elsewhere, to an unequal one, into row n-1
    pos = None
    for i in real[len(real) // 2:]:
        for k in range(3):
            v = M.w[k][i]
            eq = [(r, w) for w in range(3) for r in range(rows) if M.w[w][r] == v and (r, w) != (i, k) and (r, w) != M.target(M.maps[k][i])]
            if eq:
                pos = (i, k, eq[0])
                break
        if pos:
            break
    if pos:
        i, k, (r, w) = pos
        out.append(Case("redirect_equal", with_mapping(state, k, i, r | (w << 30)), circuit_changed=True))
    i, k = mid
    uneq = next((r, w) for r in range(rows) for w in range(3) if M.w[w][r] != M.w[k][i])
    out.append(Case("redirect_unequal", with_mapping(state, k, i, uneq[0] | (uneq[1] << 30)), circuit_changed=True))
    out.append(Case("redirect_row_n-1", with_mapping(state, k, i, (n - 1) | (k << 30)), circuit_changed=True))
    return out
