"""Shared cases of the tests of the layout entries of the check of KZG cell proofs (tests/test_kzg_check_layout_host.py,
tests/test_gpu_kzg_check_layout.py; test infrastructure).  Everything is built from tests/kzg_check_cells_cases.py: a layout of S commitments is a world
of 8 polynomials with commitments[c] = base[c % 8], and a cell of label c is a cell of polynomial c % 8 -- no test needs more than 8 host MSMs."""
import numpy as np

from oracle.pyoracle import aligned_copy
from tests.kzg_check_cells_cases import make_world

BASE = 8  # polynomials of a world
MAX_S = 1 << 16  # BBGPU_KZG_CHECK_MAX_LAYOUT_COMMITMENTS
PIECE = 1024  # KZG_LAYOUT_PIECE (csrc/bbgpu_internal.h): cells per wave of the grouped fold
FOLD_RANGE = 4096  # KZG_FOLD_RANGE


def make_worlds(lib, oracle, tmp_path_factory):
    """one world of 8 polynomials per (n, l), made on first use, never written to"""
    made = {}

    def world(n, l):
        if (n, l) not in made:
            made[(n, l)] = make_world(lib, oracle, tmp_path_factory.mktemp("layout_%d_%d" % (n, l)), n, l, BASE)
        return made[(n, l)]
    return world


def commitments_of(W, S):
    """the S commitments of a layout over the world's polynomials: commitments[c] = base[c % batch]"""
    return aligned_copy(W["commitments"][np.arange(S) % W["batch"]])


def cells_under(W, labels, start=0):
    """one true cell per label, in the labelled form: cell t carries labels[t] and is a cell of polynomial labels[t] % batch, the cell indices scrambled
    as tests.kzg_check_cells_cases.cells_of scrambles them (it is this function at labels[t] = t % batch): (which, cell, values (count * l, 4), proofs)"""
    labels = np.asarray(labels, dtype=np.int64)
    t = np.arange(start, start + len(labels))
    b, k = labels % W["batch"], (t * 7 + t // W["batch"]) % W["m"]
    idx = k[:, None] + W["m"] * np.arange(W["l"])[None, :]
    return labels.astype(np.uint32), k.astype(np.uint32), aligned_copy(W["values"][b[:, None], idx].reshape(-1, 4)), aligned_copy(W["proofs"][b, k])


def uniform(S, count):
    """labels spread over all of 0 .. S - 1 (cells of every polynomial follow one another as in cells_of)"""
    return (np.arange(count) * 5 + np.arange(count) // S) % S


def mixed(S, count):
    """mixed labels with duplicates that leave every label = 3 mod 5 without a cell"""
    lab = (np.arange(count) * 11 + 7) % S
    lab[lab % 5 == 3] -= 1
    return lab


def patterns(S, count):
    """the label patterns of the device tests"""
    out = {"uniform": uniform(S, count), "one_label": np.full(count, S - 1)}
    long = uniform(S, count)
    long[300:300 + FOLD_RANGE + 1] = min(70, S - 1)  # one list of 4097 cells (five pieces, one of a single cell), the rest spread
    out["one_long_list"] = long
    if S > 4096:
        out["below_64"] = np.arange(count) % 64
    return out


def rows_world(W, batch):
    """the world as a layout of `batch` rows in the open-cosets form: row c is polynomial c % 8"""
    idx = np.arange(batch) % W["batch"]
    return dict(W, batch=batch, commitments=aligned_copy(W["commitments"][idx]), values=W["values"][idx], proofs=aligned_copy(W["proofs"][idx]))
