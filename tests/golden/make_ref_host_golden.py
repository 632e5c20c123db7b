#!/usr/bin/env python3
"""Golden vectors for the oracle's host-side restatement: seeded inputs and what the REFERENCE's own host C++
computes for them.

Run in the build container only: needs oracle/_ref/libref_host.so (the reference's host sources compiled where they
lie, `make -C oracle ref`; never copied, never shipped).  Writes DATA only:

  ref_host_kat.npz  per case of tests/test_oracle_vs_ref.py: the inputs (arrays; input files as bytes) and the
                    reference's outputs (arrays; output files as bytes); plus the `.dim/.means/.stds/.modes` the
                    reference's prep writes for the PLINK set of tests/test_gpu_workflow_chain.py (with the sha256 of
                    that set, so a changed generator is reported as such)

Usage: PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_ref_host_golden.py [oracle/_ref/libref_host.so]
"""
import ctypes as C
import hashlib
import os
import shutil
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.dont_write_bytecode = True
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
SO = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "oracle", "_ref", "libref_host.so")

import cigwas_amd.synth as synth  # noqa: E402
import test_gpu_workflow_chain as chain_test  # noqa: E402
import test_oracle_vs_ref as T  # noqa: E402  (case inputs and file writers shared with the tests)

GOLDEN = os.path.join(HERE, "files")


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _bytes(path):
    return np.frombuffer(open(path, "rb").read(), np.uint8)


def main():
    L = C.CDLL(SO)
    for f in ("ref_subset_variables", "ref_load_mxm", "ref_load_pxp", "ref_load_mxp", "ref_read_blocks", "ref_load_phen",
              "ref_block_chr"):
        getattr(L, f).restype = C.c_int
    L.ref_load_pxp.argtypes = [C.c_char_p, C.c_char_p, C.c_float, C.c_void_p, C.c_void_p]
    L.ref_hanning_smoothing.restype = None
    L.ref_prep.restype = None
    out = {}
    tmp = tempfile.mkdtemp()
    try:
        # subset_variables
        for seed in T.SUBSET_SEEDS:
            G, n, p = T.subset_case(seed)
            out[f"subset/{seed}/G"] = G
            for depth in T.SUBSET_DEPTHS:
                o = np.zeros(n, np.int32)
                cnt = L.ref_subset_variables(_p(G), n, n - p, depth, _p(o))
                out[f"subset/{seed}/d{depth}"] = o[:cnt].copy()
        # reduce_gcs / reduce_gc result files
        for seed in T.GCS_SEEDS:
            for use_map in (False, True):
                k = f"gcs/{seed}/{int(use_map)}"
                G, Cm, S, P, imap, n, p, ml = T.gcs_case(seed, use_map)
                for name, a in (("G", G), ("C", Cm), ("S", S), ("P", P)):
                    out[f"{k}/{name}"] = a
                if use_map:
                    out[f"{k}/imap"] = imap
                base = os.path.join(tmp, "gcs")
                L.ref_reduce_gcs_to_file(_p(G), _p(Cm), _p(S), _p(P), len(P), n, p, ml, _p(imap) if use_map else None, base.encode())
                for ext in ("mdim",) + T.EXTS + ("sep",):
                    out[f"{k}/{ext}"] = _bytes(base + "." + ext)
        for use_map in (False, True):
            k = f"gc/{int(use_map)}"
            G, Cm, Nm, P, imap, n, p = T.gc_case(use_map)
            for name, a in (("G", G), ("C", Cm), ("N", Nm), ("P", P)):
                out[f"{k}/{name}"] = a
            if use_map:
                out[f"{k}/imap"] = imap
            base = os.path.join(tmp, "gc")
            L.ref_reduce_gc_to_file(_p(G), _p(Cm), _p(Nm), _p(P), len(P), n, p, 14, _p(imap) if use_map else None, base.encode())
            for ext in ("mdim",) + T.EXTS:
                out[f"{k}/{ext}"] = _bytes(base + "." + ext)
        # loaders on the reference's own fixtures
        g = lambda f: os.path.join(GOLDEN, f).encode()  # noqa: E731
        m = L.ref_load_mxm(g("small_mxm.bin"), None)
        buf = np.zeros(m * m, np.float32)
        L.ref_load_mxm(g("small_mxm.bin"), _p(buf))
        out["load/mxm"] = buf.reshape(m, m)
        corr, ess = np.zeros(9, np.float32), np.zeros(9, np.float32)
        out["load/pxp_p"] = np.array([L.ref_load_pxp(g("trait_summary_stats.txt"), None, 500000.0, _p(corr), _p(ess))])
        out["load/pxp_corr"], out["load/pxp_ess"] = corr.reshape(3, 3), ess.reshape(3, 3)
        nph = C.c_int()
        corr = np.zeros(9, np.float32)
        nm = L.ref_load_mxp(g("marker_trait_summary_stats.txt"), None, None, 0, b"1", 0, 2, 0, _p(corr), None, C.byref(nph))
        out["load/mxp_block_counts"], out["load/mxp_block_corr"] = np.array([nm, nph.value]), corr.reshape(nm, 3)
        ix = np.fromfile(os.path.join(GOLDEN, "marker_indices.bin"), np.int32)
        corr = np.zeros(len(ix) * 3, np.float32)
        nm = L.ref_load_mxp(g("marker_trait_summary_stats.txt"), None, _p(ix), len(ix), b"", 0, 0, 0, _p(corr), None, C.byref(nph))
        out["load/mxp_ix_count"], out["load/mxp_ix_corr"] = np.array([nm]), corr.reshape(nm, 3)
        f, l_, o = (np.zeros(8, np.int32) for _ in range(3))
        nb = L.ref_read_blocks(g("test.blocks"), _p(f), _p(l_), _p(o), 8)
        out["load/blocks"] = np.stack([f[:nb], l_[:nb], o[:nb]], axis=1)
        ns = L.ref_load_phen(g("with_nan.phen"), None, C.byref(nph))
        data = np.zeros(ns * nph.value, np.float32)
        L.ref_load_phen(g("with_nan.phen"), _p(data), C.byref(nph))
        out["load/phen_shape"], out["load/phen"] = np.array([ns, nph.value]), data
        # hetcor loaders with standard errors
        c, se, mc, ms = T.het_case()
        out["het/c"], out["het/se"], out["het/mc"], out["het/ms"] = c, se, mc, ms
        paths = T.write_het_files(tmp, c, se, mc, ms)
        p = c.shape[0]
        corr, ess = np.zeros(p * p, np.float32), np.zeros(p * p, np.float32)
        L.ref_load_pxp(paths["pxp"].encode(), paths["pxp_se"].encode(), 0.0, _p(corr), _p(ess))
        out["het/pxp_corr"], out["het/pxp_ess"] = corr.reshape(p, p), ess.reshape(p, p)
        corr, ess = np.zeros(4 * p, np.float32), np.zeros(4 * p, np.float32)
        nm = L.ref_load_mxp(paths["mxp"].encode(), paths["mxp_se"].encode(), None, 0, b"1", 1, 4, 0, _p(corr), _p(ess), C.byref(nph))
        out["het/mxp_count"], out["het/mxp_corr"], out["het/mxp_ess"] = np.array([nm]), corr.reshape(nm, p), ess.reshape(nm, p)
        # blocking
        for seed, n, maxb in T.BLOCKING_CASES:
            k = f"blocking/{seed}"
            v = T.blocking_case(seed, n)
            out[f"{k}/v"] = v
            for ws in T.BLOCKING_WINDOWS:
                r = np.zeros(n, np.float64)
                L.ref_hanning_smoothing(_p(v), C.c_int(n), C.c_int(ws), _p(r))
                out[f"{k}/smooth{ws}"] = r
            first, last = np.zeros(n, np.int64), np.zeros(n, np.int64)
            kk = L.ref_block_chr(_p(v), C.c_int(n), C.c_int(maxb), _p(first), _p(last), C.c_int(n))
            out[f"{k}/blocks"] = np.stack([first[:kk], last[:kk]], axis=1)
        # mps prep: inputs as bytes, the reference's output files as bytes
        for which in ("small", "synthetic"):
            d = os.path.join(tmp, "prep_" + which)
            os.makedirs(d)
            stem = os.path.join(d, "x")
            if which == "small":
                for sfx in (".bed", ".bim", ".fam"):
                    shutil.copy(os.path.join(GOLDEN, "small" + sfx), stem + sfx)
            else:
                T.synthetic_prep_inputs(stem, synth)
                for sfx in (".bed", ".bim", ".fam"):
                    out[f"prep/{which}/in{sfx}"] = _bytes(stem + sfx)
            L.ref_prep(stem.encode())
            for sfx in T.PREP_SUFFIXES:
                out[f"prep/{which}/out{sfx}"] = _bytes(stem + sfx)
        # the PLINK set of the workflow chain test
        d = os.path.join(tmp, "chain")
        os.makedirs(d)
        stem = chain_test.write_chain_inputs(d, synth)["stem"]
        out["chain_prep/input_sha256"] = np.frombuffer(chain_test.plink_sha256(stem).encode(), np.uint8)
        L.ref_prep(stem.encode())
        for sfx in T.PREP_SUFFIXES:
            out[f"chain_prep/out{sfx}"] = _bytes(stem + sfx)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    dst = os.path.join(HERE, "ref_host_kat.npz")
    np.savez_compressed(dst, **out)
    print(f"wrote {dst}: {len(out)} arrays, {os.path.getsize(dst)} bytes, sha256 "
          f"{hashlib.sha256(open(dst, 'rb').read()).hexdigest()[:16]}")


if __name__ == "__main__":
    main()
