"""What tests/test_plonk_verify_multi_host.py and tests/test_gpu_plonk_verify_multi.py share: the six circuits of tests/golden/plonk_verify.json (all
under one g2_x) as keys of ONE call of bbgpu_plonk_verify_multi / bbgpu_host_plonk_verify_multi, label arrays and the batches both files use.  Built
over tests/plonk_verify_cases.fixture(); nothing here is written to after it is made."""
import functools

import numpy as np

from tests.plonk_verify_cases import fixture, row

CIRCUITS = tuple(fixture()[1])  # the fixture's order: standard/32, standard/1024, bool/14, mimc/30, extended/32, zerowire/32
R_MOD = 21888242871839275222246405745257275088548364400416034343698204186575808495617  # the order of BN254's group
Q_MOD = 21888242871839275222246405745257275088696311157297823662689037894645226208583  # BN254's base field
EVAL_W_O_SHIFTED, EVAL_Q_MIMC_COEFFICIENT = 9, 11  # the proof's evaluations, four words each from word 72 on


def index(circuit):
    return CIRCUITS.index(circuit)


def keys(names=CIRCUITS):
    """(n, widgets, vk) per circuit: what host_plonk_verify_multi takes"""
    circuits = fixture()[1]
    return [(circuits[c]["n"], circuits[c]["widgets"], circuits[c]["vk"]) for c in names]


def honest(circuit):
    return row(circuit, "none")["proof"]


def plus_one(proof, e):
    """the proof with its e-th evaluation plus one: tools/gen_plonk_verify_golden.py's plus_one_* on any circuit's proof (Montgomery: + 2^256 mod r)"""
    out = proof.copy()
    v = sum(int(out[72 + 4 * e + k]) << (64 * k) for k in range(4))
    v = (v + (1 << 256) % R_MOD) % R_MOD
    out[72 + 4 * e:76 + 4 * e] = [(v >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for k in range(4)]
    return out


@functools.lru_cache(maxsize=None)
def tampered():
    """the four tampered proofs of the GPU tests, as (circuit, bytes).  The first and third are fixture rows the reference rejected.  The fixture has
    plus_one_w_o_shifted_eval and plus_one_q_mimc_coefficient_eval for the standard circuit only, whose verifier never reads them; here the same
    change is made to the honest proofs of the circuits whose widgets DO read them (sequential_widget.cpp:122-149 and its batch evaluation term;
    mimc_widget.cpp:180-213), so the proofs are bad: one changed evaluation moves batch_evaluation and a key point's scalar, nothing else."""
    out = (("standard/32", row("standard/32", "neg_T_LO")["proof"]),
           ("extended/32", plus_one(honest("extended/32"), EVAL_W_O_SHIFTED)),
           ("bool/14", row("bool/14", "off_curve_W_R")["proof"]),
           ("mimc/30", plus_one(honest("mimc/30"), EVAL_Q_MIMC_COEFFICIENT)))
    for _, p in out:
        p.setflags(write=False)
    return out


def others_plus(r, where):
    """the honest proofs of the five circuits that are not r's, and r under its own label `where` ("first", "middle", "last"): labels, proofs, r's position"""
    names = [c for c in CIRCUITS if c != r["circuit"]]
    p = {"first": 0, "middle": len(names) // 2, "last": len(names)}[where]
    names.insert(p, r["circuit"])
    proofs = np.stack([r["proof"] if j == p else honest(c) for j, c in enumerate(names)])
    return np.array([index(c) for c in names], dtype=np.uint32), proofs, p


def honest_batch(labels):
    """one honest proof per label; the 32-gate standard circuit takes the fixture's other witnesses in turn"""
    pool = [honest("standard/32")] + [row("standard/32", "other_witness_%d" % k)["proof"] for k in range(4)]
    seen, out = 0, []
    for c in labels:
        if CIRCUITS[int(c)] == "standard/32":
            out.append(pool[seen % len(pool)])
            seen += 1
        else:
            out.append(honest(CIRCUITS[int(c)]))
    return np.stack(out)


def round_robin(count):
    return (np.arange(count) % len(CIRCUITS)).astype(np.uint32)


def sorted_then_round_robin(count, head):
    """the first `head` labels sorted by circuit (runs), the rest round-robin (gaps)"""
    return np.concatenate([np.sort(round_robin(head)), round_robin(count - head)]).astype(np.uint32)


def place(labels, proofs, position, bad):
    """the batch with the tampered proof `bad` = (circuit, bytes) at `position`, under its own circuit's label"""
    labels, proofs = labels.copy(), proofs.copy()
    labels[position] = index(bad[0])
    proofs[position] = bad[1]
    return labels, proofs


def other_g2():
    """-(x G2): another finite point of order r on the twist, so another reference string's g2_x as far as a handle can tell"""
    out = fixture()[0].copy()
    for c in (2, 3):  # y = (c0, c1); the negative of a Montgomery residue is the residue of the negative
        v = sum(int(out[4 * c + k]) << (64 * k) for k in range(4)) % Q_MOD
        out[4 * c:4 * c + 4] = [((Q_MOD - v) % Q_MOD >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for k in range(4)]
    return out
