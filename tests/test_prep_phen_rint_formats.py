"""No GPU: the rule of cusk_phen_rint (include/cusk_hip.h) restated in numpy float64 -- scipy.stats.rankdata(method="average")
on the observed values, scipy.special.ndtri, mean and population sd -- pinned on a case worked by hand; the key map of
csrc/rint_math.h restated in numpy; the new symbols; and the command lines of `prep-phen --rint`.
tests/test_gpu_prep_phen_rint.py imports rint_restated and key_restated as its references."""
import argparse
import math
import os
import re

import numpy as np
import pytest
from scipy.special import ndtri
from scipy.stats import rankdata

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, TOO_FEW = 0, 2


def rint_restated(vals, select=None, offset=0.375):
    """dict(out float64 p x N, n, mean, sd, status, rank2 int64 p x N) of the rule's steps 1-6.  -0.0 == +0.0 as floats, so
    rankdata ties them; a trait that is not selected passes through with n = its count of finite values."""
    vals = np.atleast_2d(np.asarray(vals, np.float32))
    p, N = vals.shape
    select = np.ones(p, bool) if select is None else np.asarray(select).astype(bool)
    out = np.full((p, N), np.nan)
    rank2 = np.zeros((p, N), np.int64)
    n, status = np.zeros(p, np.int32), np.zeros(p, np.int32)
    mean, sd = np.full(p, np.nan), np.full(p, np.nan)
    for t in range(p):
        U = np.isfinite(vals[t])
        n[t] = U.sum()
        if not select[t]:
            out[t] = vals[t].astype(np.float64)
            continue
        if n[t]:
            r = rankdata(vals[t, U].astype(np.float64), method="average")
            rank2[t, U] = np.rint(2 * r).astype(np.int64)
            q = ndtri((r - offset) / (n[t] + 1 - 2 * offset))
            m, s = q.mean(), q.std()
        if n[t] < 2 or not s > 0.0:
            status[t] = TOO_FEW
            continue
        mean[t], sd[t] = m, s
        out[t, U] = (q - m) / s
    return {"out": out, "n": n, "mean": mean, "sd": sd, "status": status, "rank2": rank2}


def key_restated(v):
    """the order-preserving uint32 image of float32 values: -0.0 on +0.0, missing (NaN, +-Inf) on 0xFFFFFFFF"""
    v = np.ascontiguousarray(v, np.float32)
    bits = v.view(np.uint32).copy()
    bits[bits == 0x80000000] = 0
    key = np.where(bits & 0x80000000, ~bits, bits | np.uint32(0x80000000)).astype(np.uint32)
    key[~np.isfinite(v)] = 0xFFFFFFFF
    return key


def test_restated_rule_on_a_hand_worked_case():
    """Five observed values with one tie, and one NA.  Sorted: -1 < 0 < 2.5 = 2.5 < 7, ranks 1, 2, 3.5, 3.5, 5; with Blom's
    offset the probabilities are (r - 3/8) / (5 + 1/4) = 0.625 / 5.25, 1.625 / 5.25, 3.125 / 5.25, 4.625 / 5.25."""
    vals = np.array([[2.5, -1.0, np.nan, 0.0, 2.5, 7.0]], np.float32)
    ref = rint_restated(vals)
    assert ref["n"][0] == 5 and ref["status"][0] == OK
    assert list(ref["rank2"][0]) == [7, 2, 0, 4, 7, 10]
    probs = np.array([3.125, 0.625, 1.625, 3.125, 4.625]) / 5.25
    q = np.array([0.24104039388602685, -1.1797611176118612, -0.49720057068155404, 0.24104039388602685, 1.1797611176118612])
    for qi, pi in zip(q, probs):  # the scores by their defining property, without ndtri
        assert abs(0.5 * math.erfc(-qi / math.sqrt(2.0)) - pi) < 1e-15
    assert q[1] == -q[4]  # 0.625 / 5.25 and 4.625 / 5.25 are symmetric about 1/2
    m, s = -0.0030239565819000893, 0.7933519040307465
    assert abs(sum(q) / 5 - m) < 1e-16 and abs(math.sqrt(sum((x - m) ** 2 for x in q) / 5) - s) < 1e-15
    assert abs(ref["mean"][0] - m) < 1e-15 and abs(ref["sd"][0] - s) < 1e-15
    seen = [0, 1, 3, 4, 5]
    assert np.allclose(ref["out"][0, seen], (q - m) / s, rtol=0, atol=1e-14) and np.isnan(ref["out"][0, 2])
    assert ref["out"][0, 0] == ref["out"][0, 4]
    # offsets 0 and 1/2: r / (n + 1) and (r - 1/2) / n
    assert np.allclose(rint_restated(vals, offset=0.0)["out"][0, 1], (ndtri(1 / 6) - ndtri(np.array([3.5, 1, 2, 3.5, 5]) / 6).mean())
                       / ndtri(np.array([3.5, 1, 2, 3.5, 5]) / 6).std(), rtol=0, atol=1e-14)
    assert np.allclose(rint_restated(vals, offset=0.5)["sd"][0], ndtri((np.array([3.5, 1, 2, 3.5, 5]) - 0.5) / 5).std(), rtol=0, atol=1e-15)
    # status and pass-through
    odd = np.array([[4.0, 4.0, 4.0, np.nan], [np.nan, 1.0, np.nan, np.inf], [3.0, np.nan, -np.inf, 1.0]], np.float32)
    ref = rint_restated(odd, select=[1, 1, 0])
    assert list(ref["status"]) == [TOO_FEW, TOO_FEW, OK] and list(ref["n"]) == [3, 1, 2]
    assert np.all(np.isnan(ref["out"][:2])) and np.all(np.isnan(ref["mean"])) and np.all(np.isnan(ref["sd"]))
    assert list(ref["rank2"][0]) == [4, 4, 4, 0] and list(ref["rank2"][2]) == [0, 0, 0, 0]
    assert np.array_equal(ref["out"][2].astype(np.float32).view(np.uint32), odd[2].view(np.uint32))
    # -0.0 and +0.0 tie
    assert list(rint_restated(np.array([[-0.0, 0.0, 1.0]], np.float32))["rank2"][0]) == [3, 3, 6]


def test_key_map_is_order_preserving_on_specials():
    den = np.float32(1e-45)
    fmax, fmin = np.finfo(np.float32).max, np.finfo(np.float32).tiny
    v = np.array([-fmax, -1.0, -fmin, -2 * den, -den, 0.0, den, 2 * den, fmin, 1.0, np.nextafter(np.float32(1), np.float32(2)), fmax], np.float32)
    assert np.all(np.diff(v.astype(np.float64)) > 0)
    k = key_restated(v)
    assert np.all(np.diff(k.astype(np.int64)) > 0)
    assert key_restated(np.array([-0.0], np.float32))[0] == key_restated(np.array([0.0], np.float32))[0] == 0x80000000
    assert k[-1] == 0xFF7FFFFF and k[0] == 0x00800000
    assert np.all(key_restated(np.array([np.nan, -np.nan, np.inf, -np.inf], np.float32)) == 0xFFFFFFFF)
    rng = np.random.default_rng(5)
    x = rng.integers(0, 2 ** 32, 100000, dtype=np.uint64).astype(np.uint32).view(np.float32)
    x = x[np.isfinite(x)]
    order = np.argsort(x, kind="stable")
    kx = key_restated(x)[order].astype(np.int64)
    assert np.all(np.diff(kx) >= 0) and np.array_equal(np.diff(kx) == 0, np.diff(x[order]) == 0)


NEW_SYMBOLS = ("cusk_phen_rint", "cusk_phen_rint_timing", "cusk_phen_rint_tile")


def test_symbols_exist_with_the_headers_signatures():
    from cigwas_amd._lib import SYMBOLS, lib

    header = open(os.path.join(ROOT, "include", "cusk_hip.h")).read()
    L = lib()
    for name in NEW_SYMBOLS:
        assert name in SYMBOLS and hasattr(L, name), name
        decl = re.search(r"\b" + name + r"\(([^;]*?)\);", header, re.S)
        assert decl, name
        args = [a for a in decl.group(1).split(",") if a.strip() and a.strip() != "void"]
        assert len(SYMBOLS[name][1]) == len(args), (name, args)
    assert L.cusk_phen_rint(None, None, 0, 0, None, 0.375, None, None, None, None, None, None) == 2
    T = L.cusk_phen_rint_tile()
    assert T >= 64 and T & (T - 1) == 0
    L.cusk_phen_rint_timing(None, None)  # tolerated


def _args(**kw):
    base = dict(bfiles="set", table="t.tsv", out="o.phen", covar=None, ordinal=None, rint=False, rint_offset=None)
    base.update(kw)
    return argparse.Namespace(**base)


def test_argv_and_argument_errors(tmp_path):
    from cigwas_amd import cli

    head = [cli.MPS_PATH, "prep-phen", "set", "t.tsv", "o.phen"]
    assert cli.prep_phen_argv(_args()) == head + ["NULL"]  # as it is built today
    assert cli.prep_phen_argv(argparse.Namespace(bfiles="set", table="t.tsv", out="o.phen", covar="c.tsv", ordinal=None)) == head + ["c.tsv"]
    assert cli.prep_phen_argv(_args(rint=True)) == head + ["NULL", "rint"]
    assert cli.prep_phen_argv(_args(rint=True, rint_offset=0.5, covar="c.tsv")) == head + ["c.tsv", "rint=0.5"]
    assert cli.prep_phen_argv(_args(rint=True, rint_offset=0.0)) == head + ["NULL", "rint=0.0"]
    table = tmp_path / "t.tsv"
    table.write_text("IID FID a b cc\n1 1 0.5 1 0\n2 2 0.25 0 1\n3 3 NA 1 2\n")
    P = cli.build_parser()
    a = P.parse_args(["prep-phen", "set", str(table), "o.phen", "--ordinal", "b", "--rint"])
    assert a.func is cli.prep_phen and cli.prep_phen_argv(a)[5:] == ["NULL", "ordinal=2", "rint"]
    a = P.parse_args(["prep-phen", "set", str(table), "o.phen", "--rint", "--rint-offset", "0.25", "--covar", "c.tsv"])
    assert cli.prep_phen_argv(a)[5:] == ["c.tsv", "rint=0.25"]
    a = P.parse_args(["prep-phen", "set", str(table), "o.phen"])
    assert a.rint is False and a.rint_offset is None and cli.prep_phen_argv(a)[5:] == ["NULL"]
    for bad in (_args(rint_offset=0.375), _args(rint=True, rint_offset=0.51), _args(rint=True, rint_offset=-0.01),
                _args(rint=True, rint_offset=float("nan"))):
        with pytest.raises(SystemExit) as ex:
            cli.prep_phen_argv(bad)
        assert ex.value.code not in (0, None)
    with pytest.raises(SystemExit):
        P.parse_args(["prep-phen", "set", str(table), "o.phen", "--rint-offset"])
