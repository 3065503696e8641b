"""Host-side mirror of the reference's circuit front end for the resident PLONK prover (bbgpu_plonk_*).

``StandardComposer`` follows waffle::StandardComposer / ComposerBase
(src/barretenberg/waffle/composer/standard_composer.cpp:13-220, composer_base.hpp:131-199) and ``field_t`` the witness
arithmetic of plonk::stdlib::field_t (src/barretenberg/waffle/stdlib/field/field.tcc:124-252): the same gates, wire
indices, selector values and sigma mappings, so ``preprocess()`` yields exactly the state the reference's composer hands
its Prover.  Values are plain Python integers mod r here and converted to the reference's memory format (4 x u64 limbs,
Montgomery 2^256) at the end.  ``Prover`` wraps the C ABI (include/bbgpu.h); proving itself runs on the GPU only.
"""
import ctypes as C

import numpy as np

FR_MODULUS = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001
NO_WITNESS = 0xFFFFFFFF
LEFT, RIGHT, OUTPUT = 0, 1 << 30, 1 << 31  # ComposerBase::WireType, composer_base.hpp:73-79

PROOF_POINTS = ["W_L", "W_R", "W_O", "Z_1", "T_LO", "T_MID", "T_HI", "PI_Z", "PI_Z_OMEGA"]
VK_POINTS = ["SIGMA_1", "SIGMA_2", "SIGMA_3", "Q_M", "Q_L", "Q_R", "Q_O", "Q_C"]
VK_POINTS_BOOL = VK_POINTS + ["Q_BL", "Q_BR", "Q_BO"]
VK_POINTS_MIMC = VK_POINTS + ["Q_MIMC_COEFFICIENT", "Q_MIMC_SELECTOR"]
VK_POINTS_EXTENDED = VK_POINTS + ["Q_O_NEXT", "Q_BL", "Q_BR", "Q_BO"]  # ExtendedComposer: arithmetic, sequential, bool widgets
PROOF_EVALS_WIDGET = ["w_l_shifted_eval", "w_r_shifted_eval", "w_o_shifted_eval", "q_c_eval", "q_mimc_coefficient_eval"]  # waffle_types.hpp:39-43
PROOF_EVALS = ["w_l_eval", "w_r_eval", "w_o_eval", "sigma_1_eval", "sigma_2_eval", "z_1_shifted_eval", "linear_eval"]


def to_montgomery_limbs(values):
    """plain integers -> (len, 4) uint64 array of x * 2^256 mod r"""
    out = np.empty((len(values), 4), dtype=np.uint64)
    for i, v in enumerate(values):
        m = (v << 256) % FR_MODULUS
        for k in range(4):
            out[i, k] = (m >> (64 * k)) & 0xFFFFFFFFFFFFFFFF
    return out


class StandardComposer:
    def __init__(self):
        self.n = 0
        self.variables = []
        self.wire_epicycles = []
        self.w_l, self.w_r, self.w_o = [], [], []
        self.q_m, self.q_l, self.q_r, self.q_o, self.q_c = [], [], [], [], []

    # composer_base.hpp:131-136
    def add_variable(self, value):
        self.variables.append(value % FR_MODULUS)
        self.wire_epicycles.append([])
        return len(self.variables) - 1

    def get_variable(self, index):
        return self.variables[index]

    def _gate(self, a, b, c, q_m, q_l, q_r, q_o, q_c):
        self.w_l.append(a); self.w_r.append(b); self.w_o.append(c)
        self.q_m.append(q_m % FR_MODULUS); self.q_l.append(q_l % FR_MODULUS); self.q_r.append(q_r % FR_MODULUS)
        self.q_o.append(q_o % FR_MODULUS); self.q_c.append(q_c % FR_MODULUS)
        self.wire_epicycles[a].append((self.n, LEFT))
        self.wire_epicycles[b].append((self.n, RIGHT))
        self.wire_epicycles[c].append((self.n, OUTPUT))
        self.n += 1

    # standard_composer.cpp:13-36
    def create_add_gate(self, a, b, c, a_scaling, b_scaling, c_scaling, const_scaling):
        self._gate(a, b, c, 0, a_scaling, b_scaling, c_scaling, const_scaling)

    # standard_composer.cpp:38-63
    def create_mul_gate(self, a, b, c, mul_scaling, c_scaling, const_scaling):
        self._gate(a, b, c, mul_scaling, 0, 0, c_scaling, const_scaling)

    # standard_composer.cpp:65-89
    def create_bool_gate(self, a):
        self._gate(a, a, a, 1, 0, 0, -1, 0)

    # standard_composer.cpp:91-116
    def create_poly_gate(self, a, b, c, q_m, q_l, q_r, q_o, q_c):
        self._gate(a, b, c, q_m, q_l, q_r, q_o, q_c)

    # standard_composer.cpp:163-220 + composer_base.hpp:164-199 (compute_sigma_permutations)
    def preprocess(self):
        n = self.n
        log2_n = (n + 1).bit_length() - 1
        if (1 << log2_n) != n + 1:
            log2_n += 1
        new_n = 1 << log2_n
        variables = self.variables + [0]
        zero_idx = len(variables) - 1
        pad = new_n - n
        w_l = self.w_l + [zero_idx] * pad
        w_r = self.w_r + [zero_idx] * pad
        w_o = self.w_o + [zero_idx] * pad
        sel = [q + [0] * pad for q in (self.q_m, self.q_l, self.q_r, self.q_o, self.q_c)]
        sigma = [np.arange(new_n, dtype=np.uint32) + np.uint32(t) for t in (LEFT, RIGHT, OUTPUT)]
        for cyc in self.wire_epicycles:
            for j, (gate, wire) in enumerate(cyc):
                nxt_gate, nxt_wire = cyc[0] if j == len(cyc) - 1 else cyc[j + 1]
                sigma[wire >> 30][gate] = np.uint32((nxt_gate + nxt_wire) & 0xFFFFFFFF)
        return {
            "n": new_n,
            "w_l": to_montgomery_limbs([variables[i] for i in w_l]),
            "w_r": to_montgomery_limbs([variables[i] for i in w_r]),
            "w_o": to_montgomery_limbs([variables[i] for i in w_o]),
            "sigma_1_mapping": sigma[0], "sigma_2_mapping": sigma[1], "sigma_3_mapping": sigma[2],
            "q_m": to_montgomery_limbs(sel[0]), "q_l": to_montgomery_limbs(sel[1]), "q_r": to_montgomery_limbs(sel[2]),
            "q_o": to_montgomery_limbs(sel[3]), "q_c": to_montgomery_limbs(sel[4]),
        }

    def _padded_wires(self):
        """-> (w_l, w_r, w_o index lists, variables) exactly as this composer's preprocess() pads them: here the zero variable appended,
        new_n the power of two >= n + 1, padding rows pointing at it"""
        n = self.n
        log2_n = (n + 1).bit_length() - 1
        if (1 << log2_n) != n + 1:
            log2_n += 1
        pad = (1 << log2_n) - n
        zero_idx = len(self.variables)
        return [w + [zero_idx] * pad for w in (self.w_l, self.w_r, self.w_o)], self.variables + [0]

    def wire_map(self):
        """what Prover.set_wire_map / set_variables take: (w_l_index, w_r_index, w_o_index, variables_limbs) with
        variables_limbs[w_x_index] == preprocess()["w_x"] -- the loop of standard_composer.cpp:205-209 left to the GPU.  The indices are a
        property of the circuit; only variables_limbs changes from witness to witness."""
        cols, variables = self._padded_wires()
        return tuple(np.array(c, dtype=np.uint32) for c in cols) + (to_montgomery_limbs(variables),)


class BoolComposer(StandardComposer):
    """waffle::BoolComposer (composer/bool_composer.hpp:8-46, bool_composer.cpp:13-143): boolean constraints are not gates of their
    own but selectors q_bl / q_br / q_bo on the wires of the existing gates, checked by the bool widget next to the arithmetic one"""

    def __init__(self):
        super().__init__()
        self.is_bool = []
        self.zero_idx = self.add_variable(0)  # bool_composer.hpp:16

    def add_variable(self, value):
        self.is_bool.append(False)
        return super().add_variable(value)

    # bool_composer.cpp:23-29
    def create_bool_gate(self, a):
        self.is_bool[a] = True

    # bool_composer.cpp:68-143 (process_bool_gates + preprocess)
    def preprocess(self):
        n = self.n
        log2_n = (n + 1).bit_length() - 1
        if (1 << log2_n) != n + 1:
            log2_n += 1
        new_n = 1 << log2_n
        pad = new_n - n
        qb = [[1 if self.is_bool[w[i]] else 0 for i in range(n)] + [0] * pad for w in (self.w_l, self.w_r, self.w_o)]
        w_l = self.w_l + [self.zero_idx] * pad
        w_r = self.w_r + [self.zero_idx] * pad
        w_o = self.w_o + [self.zero_idx] * pad
        sel = [q + [0] * pad for q in (self.q_m, self.q_l, self.q_r, self.q_o, self.q_c)]
        sigma = [np.arange(new_n, dtype=np.uint32) + np.uint32(t) for t in (LEFT, RIGHT, OUTPUT)]
        for cyc in self.wire_epicycles:
            for j, (gate, wire) in enumerate(cyc):
                nxt_gate, nxt_wire = cyc[0] if j == len(cyc) - 1 else cyc[j + 1]
                sigma[wire >> 30][gate] = np.uint32((nxt_gate + nxt_wire) & 0xFFFFFFFF)
        v = self.variables
        return {
            "n": new_n,
            "w_l": to_montgomery_limbs([v[i] for i in w_l]), "w_r": to_montgomery_limbs([v[i] for i in w_r]),
            "w_o": to_montgomery_limbs([v[i] for i in w_o]),
            "sigma_1_mapping": sigma[0], "sigma_2_mapping": sigma[1], "sigma_3_mapping": sigma[2],
            "q_m": to_montgomery_limbs(sel[0]), "q_l": to_montgomery_limbs(sel[1]), "q_r": to_montgomery_limbs(sel[2]),
            "q_o": to_montgomery_limbs(sel[3]), "q_c": to_montgomery_limbs(sel[4]),
            "q_bl": to_montgomery_limbs(qb[0]), "q_br": to_montgomery_limbs(qb[1]), "q_bo": to_montgomery_limbs(qb[2]),
        }

    def _padded_wires(self):  # bool_composer.cpp:100-115: the composer's own zero variable pads, none is appended
        n = self.n
        log2_n = (n + 1).bit_length() - 1
        if (1 << log2_n) != n + 1:
            log2_n += 1
        pad = (1 << log2_n) - n
        return [w + [self.zero_idx] * pad for w in (self.w_l, self.w_r, self.w_o)], list(self.variables)


class MiMCComposer(StandardComposer):
    """waffle::MiMCComposer (composer/mimc_composer.hpp, mimc_composer.cpp:13-250): a MiMC round x_out = (x_in + k + c)^7 is ONE gate
    (w_l = k, w_r = (x_in + k + c)^3, w_o = x_in) whose result is the NEXT gate's output wire; gates that break the chain get a no-op
    gate in between to carry the pending output"""

    def __init__(self):
        super().__init__()
        self.q_mimc_coefficient, self.q_mimc_selector = [], []
        self.add_variable(0)
        self.zero_idx = 0
        self.current_output_wire = NO_WITNESS

    def _gate(self, a, b, c, q_m, q_l, q_r, q_o, q_c):  # every standard gate: mimc_composer.cpp:13-63
        if self.current_output_wire != NO_WITNESS:
            self.create_noop_gate()
        super()._gate(a, b, c, q_m, q_l, q_r, q_o, q_c)
        self.q_mimc_coefficient.append(0)
        self.q_mimc_selector.append(0)
        self.current_output_wire = NO_WITNESS

    def _zero_selectors(self, coefficient, selector):
        for q in (self.q_m, self.q_l, self.q_r, self.q_o, self.q_c):
            q.append(0)
        self.q_mimc_coefficient.append(coefficient % FR_MODULUS)
        self.q_mimc_selector.append(selector)

    # mimc_composer.cpp:65-90
    def create_mimc_gate(self, x_in_idx, x_cubed_idx, k_idx, x_out_idx, mimc_constant):
        if self.current_output_wire != NO_WITNESS and x_in_idx != self.current_output_wire:
            self.create_noop_gate()
        self.w_o.append(x_in_idx); self.w_l.append(k_idx); self.w_r.append(x_cubed_idx)
        self.current_output_wire = x_out_idx
        self._zero_selectors(mimc_constant, 1)
        self.wire_epicycles[k_idx].append((self.n, LEFT))
        self.wire_epicycles[x_cubed_idx].append((self.n, RIGHT))
        self.wire_epicycles[x_in_idx].append((self.n, OUTPUT))
        self.n += 1

    # mimc_composer.cpp:92-120
    def create_noop_gate(self):
        self._zero_selectors(0, 0)
        self.w_l.append(self.zero_idx); self.w_r.append(self.zero_idx)
        if self.current_output_wire != NO_WITNESS:
            self.w_o.append(self.current_output_wire)
            self.wire_epicycles[self.current_output_wire].append((self.n, OUTPUT))
            self.current_output_wire = NO_WITNESS
        else:
            self.w_o.append(self.zero_idx)
            self.wire_epicycles[self.zero_idx].append((self.n, OUTPUT))
        self.wire_epicycles[self.zero_idx].append((self.n, LEFT))
        self.wire_epicycles[self.zero_idx].append((self.n, RIGHT))
        self.n += 1

    def _close_chain(self):  # mimc_composer.cpp:170-185: a pending output wire gets a gate of its own, where only that wire is constrained
        if self.current_output_wire != NO_WITNESS:
            self.w_o.append(self.current_output_wire); self.w_l.append(self.zero_idx); self.w_r.append(self.zero_idx)
            self._zero_selectors(0, 0)
            self.wire_epicycles[self.current_output_wire].append((self.n, OUTPUT))
            self.n += 1
            self.current_output_wire = NO_WITNESS

    # mimc_composer.cpp:170-250
    def preprocess(self):
        self._close_chain()
        n = self.n
        log2_n = n.bit_length() - 1
        if (1 << log2_n) != n:
            log2_n += 1
        new_n = 1 << log2_n
        pad = new_n - n
        cols = [c + [self.zero_idx] * pad for c in (self.w_l, self.w_r, self.w_o)]
        sel = [q + [0] * pad for q in (self.q_m, self.q_l, self.q_r, self.q_o, self.q_c, self.q_mimc_selector, self.q_mimc_coefficient)]
        sigma = [np.arange(new_n, dtype=np.uint32) + np.uint32(t) for t in (LEFT, RIGHT, OUTPUT)]
        for cyc in self.wire_epicycles:
            for j, (gate, wire) in enumerate(cyc):
                nxt_gate, nxt_wire = cyc[0] if j == len(cyc) - 1 else cyc[j + 1]
                sigma[wire >> 30][gate] = np.uint32((nxt_gate + nxt_wire) & 0xFFFFFFFF)
        v = self.variables
        return {
            "n": new_n,
            "w_l": to_montgomery_limbs([v[i] for i in cols[0]]), "w_r": to_montgomery_limbs([v[i] for i in cols[1]]),
            "w_o": to_montgomery_limbs([v[i] for i in cols[2]]),
            "sigma_1_mapping": sigma[0], "sigma_2_mapping": sigma[1], "sigma_3_mapping": sigma[2],
            "q_m": to_montgomery_limbs(sel[0]), "q_l": to_montgomery_limbs(sel[1]), "q_r": to_montgomery_limbs(sel[2]),
            "q_o": to_montgomery_limbs(sel[3]), "q_c": to_montgomery_limbs(sel[4]),
            "q_mimc_selector": to_montgomery_limbs(sel[5]), "q_mimc_coefficient": to_montgomery_limbs(sel[6]),
        }

    def _padded_wires(self):  # mimc_composer.cpp:170-200: closes the chain as preprocess() does (whichever is called first), n itself is rounded up
        self._close_chain()
        n = self.n
        log2_n = n.bit_length() - 1
        if (1 << log2_n) != n:
            log2_n += 1
        pad = (1 << log2_n) - n
        return [c + [self.zero_idx] * pad for c in (self.w_l, self.w_r, self.w_o)], list(self.variables)


def mimc_circuit(num_gates, x0, k):
    """the MiMCComposer fixture circuit of oracle/plonk_driver.cpp (BB_CIRCUIT=mimc): num_gates - 2 rounds x <- (x + k + c_i)^7, then x + x0"""
    composer = MiMCComposer()
    k_idx = composer.add_variable(k)
    x, x_idx = x0 % FR_MODULUS, composer.add_variable(x0)
    x0_idx = x_idx
    for i in range(max(0, num_gates - 2)):
        c = (0x1000 + 7 * i) + ((i * i + 3) << 64) + (5 << 128)
        t0 = (x + k + c) % FR_MODULUS
        cubed = pow(t0, 3, FR_MODULUS)
        out = cubed * cubed * t0 % FR_MODULUS
        cubed_idx, out_idx = composer.add_variable(cubed), composer.add_variable(out)
        composer.create_mimc_gate(x_idx, cubed_idx, k_idx, out_idx, c)
        x, x_idx = out, out_idx
    s_idx = composer.add_variable(x + composer.get_variable(x0_idx))
    composer.create_add_gate(x_idx, x0_idx, s_idx, 1, 1, -1, 0)
    return composer


def bool_circuit(num_gates):
    """the BoolComposer fixture circuit of oracle/plonk_driver.cpp (BB_CIRCUIT=bool): num_gates / 2 pairs of bits a, b constrained
    boolean, c = a b (mul gate), d = a + c (add gate)"""
    composer = BoolComposer()
    for i in range(num_gates // 2):
        abit, bbit = (i * 7 + 1) & 1, ((i * 5 + 3) >> 1) & 1
        a, b = composer.add_variable(abit), composer.add_variable(bbit)
        c, d = composer.add_variable(abit & bbit), composer.add_variable(abit + (abit & bbit))
        composer.create_bool_gate(a)
        composer.create_bool_gate(b)
        composer.create_mul_gate(a, b, c, 1, -1, 0)
        composer.create_add_gate(a, c, d, 1, 1, -1, 0)
    return composer


class field_t:
    """plonk::stdlib::field_t: value = multiplicative_constant * witness + additive_constant (field.tcc:11-37)"""

    def __init__(self, composer, witness_index=NO_WITNESS, additive_constant=0, multiplicative_constant=1):
        self.context = composer
        self.witness_index = witness_index
        self.additive_constant = additive_constant % FR_MODULUS
        self.multiplicative_constant = multiplicative_constant % FR_MODULUS

    @staticmethod
    def witness(composer, value):
        return field_t(composer, composer.add_variable(value))

    @staticmethod
    def constant(composer, value):
        return field_t(composer, NO_WITNESS, value, 0)

    # field.tcc:124-181
    def __add__(self, other):
        ctx = self.context
        if self.witness_index == other.witness_index:
            return field_t(ctx, self.witness_index, self.additive_constant + other.additive_constant,
                           self.multiplicative_constant + other.multiplicative_constant)
        if self.witness_index != NO_WITNESS and other.witness_index == NO_WITNESS:
            return field_t(ctx, self.witness_index, self.additive_constant + other.additive_constant, self.multiplicative_constant)
        if self.witness_index == NO_WITNESS and other.witness_index != NO_WITNESS:
            return field_t(ctx, other.witness_index, self.additive_constant + other.additive_constant, other.multiplicative_constant)
        left, right = ctx.get_variable(self.witness_index), ctx.get_variable(other.witness_index)
        out = (left * self.multiplicative_constant + right * other.multiplicative_constant + self.additive_constant + other.additive_constant) % FR_MODULUS
        res = field_t(ctx, ctx.add_variable(out))
        ctx.create_add_gate(self.witness_index, other.witness_index, res.witness_index, self.multiplicative_constant,
                            other.multiplicative_constant, -1, self.additive_constant + other.additive_constant)
        return res

    # field.tcc:192-252
    def __mul__(self, other):
        ctx = self.context
        if self.witness_index == NO_WITNESS and other.witness_index == NO_WITNESS:
            return field_t(ctx, NO_WITNESS, self.additive_constant * other.additive_constant, 1)
        if self.witness_index != NO_WITNESS and other.witness_index == NO_WITNESS:
            return field_t(ctx, self.witness_index, self.additive_constant * other.additive_constant,
                           self.multiplicative_constant * other.additive_constant)
        if self.witness_index == NO_WITNESS and other.witness_index != NO_WITNESS:
            return field_t(ctx, other.witness_index, self.additive_constant * other.additive_constant,
                           other.multiplicative_constant * self.additive_constant)
        q_c = self.additive_constant * other.additive_constant % FR_MODULUS
        q_r = self.additive_constant * other.multiplicative_constant % FR_MODULUS
        q_l = self.multiplicative_constant * other.additive_constant % FR_MODULUS
        q_m = self.multiplicative_constant * other.multiplicative_constant % FR_MODULUS
        left, right = ctx.get_variable(self.witness_index), ctx.get_variable(other.witness_index)
        out = (left * right * q_m + left * q_l + right * q_r + q_c) % FR_MODULUS
        res = field_t(ctx, ctx.add_variable(out))
        ctx.create_poly_gate(self.witness_index, other.witness_index, res.witness_index, q_m, q_l, q_r, -1, q_c)
        return res


def bench_circuit(num_gates, a0, b0):
    """the add/mul chain of the reference's PLONK benchmark (src/barretenberg/test/benchmarks/bench_plonk.cpp:25-37) with given
    plain witness values; returns the composer"""
    composer = StandardComposer()
    a, b = field_t.witness(composer, a0), field_t.witness(composer, b0)
    for _ in range(num_gates // 4 - 4):
        c = a + b
        c = a * c
        a = b * b
        b = c * c
    return composer


def zero_wire_circuit(num_gates, a0):
    """a * 0 = 0 in every gate: w_r and w_o are identically zero, so the wire commitments W_R and W_O are the point at infinity
    (mirror of build_zero_wire_circuit in oracle/plonk_driver.cpp; tests/golden/infinity_commitments.json)"""
    composer = StandardComposer()
    zero_idx = composer.add_variable(0)
    a = a0 % FR_MODULUS
    for _ in range(num_gates):
        ai = composer.add_variable(a)
        composer.create_mul_gate(ai, zero_idx, zero_idx, 1, -1, 0)
        a = (a * a + 1) % FR_MODULUS
    return composer


class _Circuit(C.Structure):
    _fields_ = [("n", C.c_size_t)] + [(k, C.c_void_p) for k in ("w_l", "w_r", "w_o", "sigma_1_mapping", "sigma_2_mapping", "sigma_3_mapping",
                                                               "q_m", "q_l", "q_r", "q_o", "q_c", "q_bl", "q_br", "q_bo",
                                                               "q_mimc_selector", "q_mimc_coefficient", "q_o_next")]


FAIL_KINDS = {"ARITH": 1, "BOOL_L": 2, "BOOL_R": 4, "BOOL_O": 8, "MIMC_CUBE": 16, "MIMC_OUT": 32}  # BBGPU_PLONK_FAIL_*
NONE = 0xFFFFFFFF  # BBGPU_PLONK_NONE


class WitnessError(Exception):
    """construct_proof / construct_proofs with set_witness_check(True): a witness does not satisfy the circuit and no proof was written.
    ``reports`` holds one report dict per lane (one for the single proof); a lane is good iff gate_failures == copy_failures == 0."""

    def __init__(self, message, reports):
        super().__init__(message)
        self.reports = reports

    def bad_lanes(self):
        return [j for j, r in enumerate(self.reports) if r["gate_failures"] or r["copy_failures"]]


def _circuit_struct(state):
    """-> (_Circuit, the arrays it points into)"""
    n = int(state["n"])
    keep = {k: np.ascontiguousarray(state[k]) for k in state if k != "n"}
    c = _Circuit()
    c.n = n
    for k, a in keep.items():
        want = np.uint32 if k.endswith("mapping") else np.uint64
        assert a.dtype == want and a.shape[0] == n, k
        setattr(c, k, a.ctypes.data)
    return c, keep


def host_check_witness(state, lib=None):
    """bbgpu_host_plonk_check_witness: does the witness state["w_l" / "w_r" / "w_o"] satisfy the circuit `state` (rows 0 .. n-2: include/bbgpu.h)?
    Host arithmetic, no GPU.  -> report dict"""
    from .bbgpu import BbGpu, WitnessReport
    if lib is None:
        lib = BbGpu(init=False)
    c, keep = _circuit_struct(state)
    rep = WitnessReport()
    lib.lib.bbgpu_host_plonk_check_witness.argtypes = [C.POINTER(_Circuit), C.POINTER(WitnessReport)]
    lib._chk(lib.lib.bbgpu_host_plonk_check_witness(C.byref(c), C.byref(rep)))
    del keep
    return rep.as_dict()


def variables_from_wires(w_l, w_r, w_o):
    """any expanded witness -> ((w_l_index, w_r_index, w_o_index), variables): the distinct 32-byte rows of the three wire vectors are the
    variables, every cell the index of its row.  For states that come without a composer (tests/golden/plonk_extended_state.npz); a composer's
    own wire_map() keeps the composer's numbering instead."""
    cols = [np.ascontiguousarray(a, dtype=np.uint64).reshape(-1, 4) for a in (w_l, w_r, w_o)]
    n = cols[0].shape[0]
    variables, inverse = np.unique(np.concatenate(cols), axis=0, return_inverse=True)
    inverse = np.asarray(inverse).reshape(-1).astype(np.uint32)
    return tuple(inverse[k * n:(k + 1) * n].copy() for k in range(3)), np.ascontiguousarray(variables)


def _witness_array(a, words):
    """one array of a witness item -> (pointer, on the device?, stream, what keeps it alive): numpy arrays and CPU tensors go as host memory,
    CUDA tensors (uint64, or int64 viewed as such) as their data_ptr() with the current torch stream"""
    if hasattr(a, "data_ptr") and hasattr(a, "is_cuda"):  # a torch.Tensor
        import torch
        assert a.dtype in (torch.int64, torch.uint64), "tensors hold 64-bit limbs (uint64, or int64 viewed as such)"
        if a.is_cuda:
            a = a.contiguous()
            assert a.numel() == words, "expected %d limbs, got %d" % (words, a.numel())
            return a.data_ptr(), True, torch.cuda.current_stream(a.device).cuda_stream, a
        a = (a.view(torch.int64) if a.dtype != torch.int64 else a).numpy().view(np.uint64)
    a = np.ascontiguousarray(a, dtype=np.uint64)
    assert a.size == words, "expected %d limbs, got %d" % (words, a.size)
    return a.ctypes.data, False, None, a


class Prover:
    """waffle::Prover over the C ABI: Prover(gpu, circuit_state, srs_handle).construct_proof()"""

    def __init__(self, gpu, state, srs_handle):
        self.gpu = gpu
        L = gpu.lib
        L.bbgpu_plonk_prover_create.argtypes = [C.POINTER(_Circuit), C.c_int]
        L.bbgpu_plonk_construct_proof.argtypes = [C.c_int, C.POINTER(C.c_uint64)]
        L.bbgpu_plonk_last_challenges.argtypes = [C.c_int, C.POINTER(C.c_uint64)]
        L.bbgpu_plonk_last_timing.argtypes = [C.c_int, C.POINTER(C.c_double)]
        L.bbgpu_plonk_prover_set_witness.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        self.n = int(state["n"])
        c, self._keep = _circuit_struct(state)
        self.handle = gpu._chk(L.bbgpu_plonk_prover_create(C.byref(c), srs_handle))

    def set_witness(self, w_l, w_r, w_o):
        arrs = [np.ascontiguousarray(a, dtype=np.uint64) for a in (w_l, w_r, w_o)]
        self.gpu._chk(self.gpu.lib.bbgpu_plonk_prover_set_witness(self.handle, *[a.ctypes.data for a in arrs]))

    def construct_proof(self):
        """-> (120,) uint64: nine affine commitments, seven evaluations, five widget-dependent evaluations (waffle_types.hpp:18-45)"""
        out = np.zeros(120, dtype=np.uint64)
        self._chk_witness(self.gpu.lib.bbgpu_plonk_construct_proof(self.handle, out.ctypes.data_as(C.POINTER(C.c_uint64))), 1)
        return out

    def _chk_witness(self, rc, lanes):
        """_chk of a proof call: BBGPU_ERR_WITNESS becomes a WitnessError that carries every lane's report"""
        from .bbgpu import ERR_WITNESS
        if rc == ERR_WITNESS:
            message = self.gpu.lib.bbgpu_last_error().decode()
            raise WitnessError(message, [self.last_witness_report(j) for j in range(lanes)])
        return self.gpu._chk(rc)

    def set_witness_check(self, flag):
        """bbgpu_plonk_set_witness_check: construct_proof / construct_proofs check their witnesses first and raise WitnessError (default off)"""
        self.gpu.lib.bbgpu_plonk_set_witness_check.argtypes = [C.c_int, C.c_int]
        self.gpu._chk(self.gpu.lib.bbgpu_plonk_set_witness_check(self.handle, 1 if flag else 0))

    def check_witness(self):
        """bbgpu_plonk_check_witness: the witness the prover holds -> report dict (good iff gate_failures == copy_failures == 0)"""
        from .bbgpu import WitnessReport
        rep = WitnessReport()
        self.gpu.lib.bbgpu_plonk_check_witness.argtypes = [C.c_int, C.POINTER(WitnessReport)]
        self.gpu._chk(self.gpu.lib.bbgpu_plonk_check_witness(self.handle, C.byref(rep)))
        return rep.as_dict()

    def check_witnesses(self, witnesses, raw=False):
        """bbgpu_plonk_check_witness_batch: witnesses as construct_proofs takes them -> one report dict per lane, in one resident call
        (raw: -> (reports, the bytes of the report array as the library wrote it))"""
        from .bbgpu import WitnessReport
        L = self.gpu.lib
        count = len(witnesses)
        keep = [[np.ascontiguousarray(a, dtype=np.uint64) for a in w] for w in witnesses]
        for w in keep:
            assert len(w) == 3 and all(a.size == self.n * 4 for a in w), "each witness is (w_l, w_r, w_o) of n x 4 limbs"
        cols = [(C.c_void_p * max(count, 1))(*[w[k].ctypes.data for w in keep]) for k in range(3)]
        reps = (WitnessReport * max(count, 1))()
        L.bbgpu_plonk_check_witness_batch.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(WitnessReport)]
        self.gpu._chk(L.bbgpu_plonk_check_witness_batch(self.handle, count, cols[0], cols[1], cols[2], reps))
        out = [reps[j].as_dict() for j in range(count)]
        return (out, bytes(reps)[:40 * count]) if raw else out

    def last_witness_report(self, lane=0):
        """bbgpu_plonk_last_witness_report: lane `lane` of the last checked proof call or check entry"""
        from .bbgpu import WitnessReport
        rep = WitnessReport()
        self.gpu.lib.bbgpu_plonk_last_witness_report.argtypes = [C.c_int, C.c_int, C.POINTER(WitnessReport)]
        self.gpu._chk(self.gpu.lib.bbgpu_plonk_last_witness_report(self.handle, int(lane), C.byref(rep)))
        return rep.as_dict()

    def construct_proofs(self, witnesses):
        """one proof per witness in one resident call (bbgpu_plonk_construct_proof_batch): witnesses is a sequence of (w_l, w_r, w_o), each
        (n, 4) uint64 as for set_witness -> (count, 120) uint64; row j is what set_witness(*witnesses[j]) + construct_proof() returns"""
        L = self.gpu.lib
        count = len(witnesses)
        keep = [[np.ascontiguousarray(a, dtype=np.uint64) for a in w] for w in witnesses]
        for w in keep:
            assert len(w) == 3 and all(a.size == self.n * 4 for a in w), "each witness is (w_l, w_r, w_o) of n x 4 limbs"
        cols = [(C.c_void_p * max(count, 1))(*[w[k].ctypes.data for w in keep]) for k in range(3)]
        out = np.zeros((count, 120), dtype=np.uint64)
        L.bbgpu_plonk_construct_proof_batch.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        self._chk_witness(L.bbgpu_plonk_construct_proof_batch(self.handle, count, cols[0], cols[1], cols[2], out.ctypes.data), count)
        return out

    # ---- witnesses as composer variables, from host or device memory (bbgpu_plonk_prover_set_wire_map, bbgpu_plonk_witness) ----
    def set_wire_map(self, w_l_index, w_r_index, w_o_index, num_variables):
        """the circuit's wire -> variable indices (StandardComposer.wire_map()[:3], or variables_from_wires): once per prover; a witness is then
        its variables, (num_variables, 4) uint64"""
        idx = [np.ascontiguousarray(a, dtype=np.uint32) for a in (w_l_index, w_r_index, w_o_index)]
        assert all(a.size == self.n for a in idx), "each index array has n entries"
        f = self.gpu.lib.bbgpu_plonk_prover_set_wire_map
        f.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
        self.gpu._chk(f(self.handle, idx[0].ctypes.data, idx[1].ctypes.data, idx[2].ctypes.data, int(num_variables)))
        self.num_variables = int(num_variables)

    def _describe(self, item):
        """a witness item -> (PlonkWitness, what keeps its memory alive): (w_l, w_r, w_o) or one variables array; numpy arrays, CPU tensors
        (host) or CUDA tensors (device, current torch stream)"""
        from .bbgpu import PlonkWitness
        d = PlonkWitness()
        if isinstance(item, (tuple, list)):
            assert len(item) == 3, "an expanded witness is (w_l, w_r, w_o)"
            got = [_witness_array(a, self.n * 4) for a in item]
            assert len({g[1] for g in got}) == 1, "w_l, w_r and w_o of one witness live in one place"
            d.form, (d.w_l, d.w_r, d.w_o) = PlonkWitness.WIRES, [g[0] for g in got]
        else:
            nv = getattr(self, "num_variables", None)
            if nv is None:  # the library answers (BBGPU_ERR_STATE); only the size is unknown here
                nv = (item.numel() if hasattr(item, "numel") else np.asarray(item).size) // 4
            got = [_witness_array(item, nv * 4)]
            d.form, d.variables = PlonkWitness.VARIABLES, got[0][0]
        d.where = PlonkWitness.DEVICE if got[0][1] else PlonkWitness.HOST
        d.hip_stream = got[0][2]
        return d, [g[3] for g in got]

    def _describe_all(self, items):
        from .bbgpu import PlonkWitness
        pairs = [self._describe(it) for it in items]
        descs = (PlonkWitness * max(len(pairs), 1))(*[p[0] for p in pairs])
        return descs, [p[1] for p in pairs]

    def set_witness_from(self, item):
        """bbgpu_plonk_prover_set_witness_from: the witness the prover holds, from (w_l, w_r, w_o) or a variables array, numpy or torch"""
        from .bbgpu import PlonkWitness
        d, keep = self._describe(item)
        f = self.gpu.lib.bbgpu_plonk_prover_set_witness_from
        f.argtypes = [C.c_int, C.POINTER(PlonkWitness)]
        self.gpu._chk(f(self.handle, C.byref(d)))
        del keep

    def set_variables(self, v):
        """set_witness for a witness given as its composer variables (needs set_wire_map)"""
        assert not isinstance(v, (tuple, list)), "one (num_variables, 4) array"
        self.set_witness_from(v)

    def construct_proofs_from(self, items):
        """construct_proofs for witnesses in any form and place, mixed freely: each item is (w_l, w_r, w_o) or one variables array, each array
        numpy / a CPU tensor (host) or a CUDA tensor (device memory, ordered behind the current torch stream) -> (count, 120) uint64"""
        from .bbgpu import PlonkWitness
        descs, keep = self._describe_all(items)
        out = np.zeros((len(items), 120), dtype=np.uint64)
        f = self.gpu.lib.bbgpu_plonk_construct_proof_batch_from
        f.argtypes = [C.c_int, C.c_int, C.POINTER(PlonkWitness), C.c_void_p]
        self._chk_witness(f(self.handle, len(items), descs, out.ctypes.data), len(items))
        del keep
        return out

    def check_witnesses_from(self, items, raw=False):
        """check_witnesses for witnesses in any form and place (see construct_proofs_from) -> one report dict per lane"""
        from .bbgpu import PlonkWitness, WitnessReport
        descs, keep = self._describe_all(items)
        count = len(items)
        reps = (WitnessReport * max(count, 1))()
        f = self.gpu.lib.bbgpu_plonk_check_witness_batch_from
        f.argtypes = [C.c_int, C.c_int, C.POINTER(PlonkWitness), C.POINTER(WitnessReport)]
        self.gpu._chk(f(self.handle, count, descs, reps))
        del keep
        out = [reps[j].as_dict() for j in range(count)]
        return (out, bytes(reps)[:40 * count]) if raw else out

    def batch_challenges(self, lane):
        """challenges() of lane `lane` of the last construct_proofs call"""
        out = np.zeros(20, dtype=np.uint64)
        self.gpu.lib.bbgpu_plonk_batch_challenges.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_uint64)]
        self.gpu._chk(self.gpu.lib.bbgpu_plonk_batch_challenges(self.handle, int(lane), out.ctypes.data_as(C.POINTER(C.c_uint64))))
        return {k: out[4 * i:4 * i + 4] for i, k in enumerate(("beta", "gamma", "alpha", "z", "nu"))}

    def batch_timing(self):
        """timing() of the last construct_proofs call, for the whole batch"""
        buf = (C.c_double * 4)()
        self.gpu.lib.bbgpu_plonk_last_batch_timing.argtypes = [C.c_int, C.POINTER(C.c_double)]
        self.gpu._chk(self.gpu.lib.bbgpu_plonk_last_batch_timing(self.handle, buf))
        return {"total_ms": buf[0], "commitments_ms": buf[1], "rest_ms": buf[2], "first_use_preparation_ms": buf[3]}

    def preprocess(self):
        """waffle::preprocess(prover): -> dict of the eight verification-key commitments, each (8,) uint64 affine"""
        out = np.zeros(96, dtype=np.uint64)
        self.gpu.lib.bbgpu_plonk_preprocess.argtypes = [C.c_int, C.POINTER(C.c_uint64)]
        self.gpu._chk(self.gpu.lib.bbgpu_plonk_preprocess(self.handle, out.ctypes.data_as(C.POINTER(C.c_uint64))))
        names = VK_POINTS_EXTENDED if "q_o_next" in self._keep else VK_POINTS_BOOL if "q_bl" in self._keep else \
            VK_POINTS_MIMC if "q_mimc_selector" in self._keep else VK_POINTS
        return {k: out[8 * i:8 * i + 8] for i, k in enumerate(names)}

    def challenges(self):
        out = np.zeros(20, dtype=np.uint64)
        self.gpu._chk(self.gpu.lib.bbgpu_plonk_last_challenges(self.handle, out.ctypes.data_as(C.POINTER(C.c_uint64))))
        return {k: out[4 * i:4 * i + 4] for i, k in enumerate(("beta", "gamma", "alpha", "z", "nu"))}

    def timing(self):
        buf = (C.c_double * 4)()
        self.gpu._chk(self.gpu.lib.bbgpu_plonk_last_timing(self.handle, buf))
        return {"total_ms": buf[0], "commitments_ms": buf[1], "rest_ms": buf[2], "first_use_preparation_ms": buf[3]}

    def destroy(self):
        if self.handle is not None:
            self.gpu.lib.bbgpu_plonk_prover_destroy(self.handle)
            self.handle = None


def hex4(limbs):
    return "%016x%016x%016x%016x" % (int(limbs[3]), int(limbs[2]), int(limbs[1]), int(limbs[0]))


def proof_lines(n, proof, mimc=False, sequential=False):
    """the text form oracle/plonk_driver.cpp prints and tests/golden/plonk_proofs.json stores (with the MiMC widget: two more evaluations,
    with the sequential widget: w_o_shifted_eval)"""
    out = ["n %d" % n]
    for i, name in enumerate(PROOF_POINTS):
        out.append("%s.x %s" % (name, hex4(proof[8 * i:8 * i + 4])))
        out.append("%s.y %s" % (name, hex4(proof[8 * i + 4:8 * i + 8])))
    for i, name in enumerate(PROOF_EVALS):
        out.append("%s %s" % (name, hex4(proof[72 + 4 * i:76 + 4 * i])))
    if mimc or sequential:
        for name in ("w_o_shifted_eval", "q_mimc_coefficient_eval")[:2 if mimc else 1]:
            i = PROOF_EVALS_WIDGET.index(name)
            out.append("%s %s" % (name, hex4(proof[100 + 4 * i:104 + 4 * i])))
    return out


def proof_from_lines(lines):
    """inverse of proof_lines (standard part): -> (n, (120,) uint64)"""
    n = int(lines[0].split()[1])
    words = []
    for ln in lines[1:1 + 18 + 7]:
        h = ln.split()[1]
        words += [int(h[16 * (3 - k):16 * (4 - k)], 16) for k in range(4)]
    return n, np.array(words + [0] * 20, dtype=np.uint64)


def proof_words(lines):
    """inverse of proof_lines for every widget set: the named lines, in any number -> (n, (120,) uint64)"""
    names = [p + c for p in PROOF_POINTS for c in (".x", ".y")] + list(PROOF_EVALS) + list(PROOF_EVALS_WIDGET)
    out = np.zeros(120, dtype=np.uint64)
    n = None
    for ln in lines:
        k, v = ln.split()
        if k == "n":
            n = int(v)
        elif k in names:
            i = names.index(k)
            out[4 * i:4 * i + 4] = [int(v[16 * (3 - j):16 * (4 - j)], 16) for j in range(4)]
    return n, out


def widget_bits(state):
    """the widget set of a circuit state as bbgpu_plonk_verifier_create takes it"""
    from .bbgpu import BbGpu
    return (BbGpu.WIDGET_BOOL if "q_bl" in state else 0) | (BbGpu.WIDGET_MIMC if "q_mimc_selector" in state else 0) | \
        (BbGpu.WIDGET_SEQUENTIAL if "q_o_next" in state else 0)


class Verifier:
    """waffle::Verifier for batches of proofs of one circuit over the C ABI (bbgpu_plonk_verifier_create / bbgpu_plonk_verify_batch):
    Verifier(gpu, n, widgets, vk, g2_x).verify(proofs) -> PlonkVerifyReport; host=True runs bbgpu_host_plonk_verify_batch (no GPU needed)"""

    def __init__(self, gpu, n, widgets, vk, g2_x):
        self.gpu, self.n, self.widgets = gpu, int(n), int(widgets)
        self.vk = np.ascontiguousarray(vk, dtype=np.uint64).reshape(-1, 8).copy()
        self.g2_x = np.ascontiguousarray(g2_x, dtype=np.uint64).reshape(16).copy()
        self.handle = gpu.plonk_verifier_create(self.n, self.widgets, self.vk, self.g2_x)

    @classmethod
    def from_prover(cls, prover, g2_x):
        """the verifier of a Prover's circuit: its key by preprocess() (one GPU call), x * G2 from the SRS's transcript (BbGpu.transcript_read_g2)"""
        vk = prover.preprocess()
        return cls(prover.gpu, prover.n, widget_bits(prover._keep), np.stack(list(vk.values())), g2_x)

    def verify(self, proofs, seed=None, locate=False, host=False):
        if host:
            return self.gpu.host_plonk_verify_batch(self.n, self.widgets, self.vk, self.g2_x, proofs, seed, locate)
        return self.gpu.plonk_verify_batch(self.handle, proofs, seed, locate)

    @staticmethod
    def verify_mixed(verifiers, circuit, proofs, seed=None, locate=False, host=False):
        """a queue of proofs of several circuits in one call (bbgpu_plonk_verify_multi): proof j claims the circuit of verifiers[circuit[j]]; the
        Verifiers share one g2_x.  One pairing check for all; host=True runs bbgpu_host_plonk_verify_multi (no GPU needed)"""
        gpu = verifiers[0].gpu
        if host:
            return gpu.host_plonk_verify_multi([(v.n, v.widgets, v.vk) for v in verifiers], verifiers[0].g2_x, circuit, proofs, seed, locate)
        return gpu.plonk_verify_multi([v.handle for v in verifiers], circuit, proofs, seed, locate)

    def destroy(self):
        if self.handle is not None:
            self.gpu.plonk_verifier_destroy(self.handle)
            self.handle = None
