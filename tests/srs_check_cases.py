"""Shared cases of the SRS-check tests (tests/test_srs_check_host.py, tests/test_gpu_srs_check.py; test infrastructure, may import oracle/): the
tampers of an honest table x^i G and the report each must give.  The host and the GPU entry are judged against the same expectations."""
import numpy as np

from oracle.pyoracle import FQ, FR, aligned_copy, from_int, to_int

NONE = 0xFFFFFFFFFFFFFFFF
SEED = np.array([0x0123456789ABCDEF, 0xFEDCBA9876543210, 0x0F1E2D3C4B5A6978, 0x1122334455667788], dtype=np.uint64)
FIELDS = ("n", "bad_points", "first_bad_point", "first_is_generator", "g2_ok", "powers_checked", "powers_ok", "first_bad_power")


def rows_of(n):
    """the rows a tamper is tried at: 0, 1, n / 2, n - 1"""
    return sorted({0, 1, n // 2, n - 1} & set(range(n)))


def g2_of(lib, oracle, tmp_path, x_mont, name):
    """x * G2 the way a caller gets it: from a written transcript"""
    path = str(tmp_path / name)
    tiny = oracle.point_table(oracle.make_srs(x_mont, 2))
    lib.write_transcript(path, tiny, 2, x_mont)
    return lib.transcript_read_g2(path)


def secret_plus_one(oracle, x_mont):
    return oracle.add(FR, x_mont, oracle.const(FR, "one"))


def honest(n):
    return dict(n=n, bad_points=0, first_bad_point=NONE, first_is_generator=1, g2_ok=1, powers_checked=1 if n >= 2 else 0, powers_ok=1 if n >= 2 else 0,
                first_bad_power=NONE)


def tampers(oracle, table, n, g2_x, g2_x1, shifted_table):
    """yields (name, table, g2_x, expected fields with BBGPU_SRS_CHECK_LOCATE); `table` is the honest (2n, 8) endo table of secret x, g2_x1 the x * G2 of
    x + 1, shifted_table the table of x^(5 + i) G"""
    for k in rows_of(n):  # (a) one added to the y of row k: off the curve
        t = aligned_copy(table)
        t[2 * k, 4:8] = from_int((to_int(t[2 * k, 4:8]) + 1) % (1 << 256))
        yield "a%d" % k, t, g2_x, dict(honest(n), bad_points=1, first_bad_point=k, powers_checked=0, powers_ok=0, first_is_generator=0 if k == 0 else 1)
    for k in rows_of(n):  # (b) the y of row k negated: still on the curve
        t = aligned_copy(table)
        t[2 * k, 4:8] = oracle.neg(FQ, t[2 * k, 4:8])
        yield "b%d" % k, t, g2_x, dict(honest(n), powers_ok=0, first_bad_power=max(k, 1) - 1, first_is_generator=0 if k == 0 else 1)
    for k in rows_of(n):  # (c) rows k and k + 1 swapped
        if k > n - 3:
            continue
        t = aligned_copy(table)
        t[[2 * k, 2 * k + 1, 2 * k + 2, 2 * k + 3]] = t[[2 * k + 2, 2 * k + 3, 2 * k, 2 * k + 1]]
        yield "c%d" % k, t, g2_x, dict(honest(n), powers_ok=0, first_bad_power=max(k, 1) - 1, first_is_generator=0 if k == 0 else 1)
    yield "d", table, g2_x1, dict(honest(n), powers_ok=0, first_bad_power=0)  # (d) the x * G2 of x + 1
    bad_g2 = g2_x.copy()  # (e) x * G2 with one added to y.c0: off the twist
    bad_g2[8:12] = from_int((to_int(bad_g2[8:12]) + 1) % (1 << 256))
    yield "e", table, bad_g2, dict(honest(n), g2_ok=0, powers_checked=0, powers_ok=0)
    yield "f", shifted_table, g2_x, dict(honest(n), first_is_generator=0)  # (f) x^(5 + i) G: consecutive powers that do not start at the generator
    yield "g", table, None, dict(honest(n), g2_ok=0, powers_checked=0, powers_ok=0)  # (g) no x * G2: the curve test only


def fields(report):
    return {k: int(getattr(report, k)) for k in FIELDS}


def whole(report):
    """every field of a report, a and b included"""
    return report.as_dict()
