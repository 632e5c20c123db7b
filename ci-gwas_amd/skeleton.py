"""Host-side mirror of the reference's operator interface for the cusk path.

`Skeleton`, `hetcor_skeleton`, `threshold_array`, `hetcor_threshold`,
`cu_corr_pearson_npn` and `cu_marker_phen_corr_pearson` take and return host
numpy arrays with the reference's argument meaning
(/root/reference/cusk/include/mps/cuPC-S.h:196, hetcor-cuPC-S.h:46,
cuPC_call_prep.h:7-15, corr_host.h:38-47,92-103) and call straight through the
C ABI of libcusk_hip.so.  `Engine` is the device-resident API used by bench.py
and the mps host program (matrix stays in HBM, sparse sepsets).
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from ._lib import ML, CuskStats, lib


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def threshold_array(n: int, alpha: float) -> np.ndarray:
    out = np.zeros(ML + 1, np.float32)
    lib().cusk_threshold_array(int(n), float(np.float32(alpha)), _ptr(out))
    return out


def hetcor_threshold(alpha: float) -> float:
    return float(lib().cusk_hetcor_threshold(float(np.float32(alpha))))


def Skeleton(Cm: np.ndarray, Th: np.ndarray, maxlevel: int, want_pmax: bool = True, want_sepset: bool = True):
    """-> (G n*n int32, level, pMax n*n float32 | None, SepSet n*n*14 int32 | None)."""
    Cm = np.ascontiguousarray(Cm, np.float32)
    n = Cm.shape[0]
    G = np.ones((n, n), np.int32)
    pmax = np.zeros((n, n), np.float32) if want_pmax else None
    sep = np.zeros((n, n, ML), np.int32) if want_sepset else None
    Th = np.ascontiguousarray(Th, np.float32)
    P, l, ml = C.c_int(n), C.c_int(0), C.c_int(int(maxlevel))
    lib().Skeleton(_ptr(Cm), C.addressof(P), _ptr(G), _ptr(Th), C.addressof(l), C.addressof(ml), _ptr(pmax), _ptr(sep))
    return G, l.value, pmax, sep


def hetcor_skeleton(Cm, G, N, th: float, maxlevel: int, time_index):
    """-> (G n*n int32 (copy, updated), level)."""
    Cm = np.ascontiguousarray(Cm, np.float32)
    n = Cm.shape[0]
    G = np.array(G, np.int32).reshape(n, n).copy()
    N = np.ascontiguousarray(N, np.float32).reshape(n, n)
    ti = np.ascontiguousarray(time_index, np.int32)
    P, l, ml, thv = C.c_int(n), C.c_int(0), C.c_int(int(maxlevel)), C.c_float(float(np.float32(th)))
    lib().hetcor_skeleton(_ptr(Cm), C.addressof(P), _ptr(G), _ptr(N), C.addressof(thv), C.addressof(l), C.addressof(ml), _ptr(ti))
    return G, l.value


def cu_marker_phen_corr_pearson(bed, phen, m, N, p, means, stds) -> np.ndarray:
    bed = np.ascontiguousarray(bed, np.uint8)
    phen = np.ascontiguousarray(phen, np.float32)
    means = np.ascontiguousarray(means, np.float32)
    stds = np.ascontiguousarray(stds, np.float32)
    out = np.zeros(m * p, np.float32)
    lib().cu_marker_phen_corr_pearson(_ptr(bed), _ptr(phen), m, N, p, _ptr(means), _ptr(stds), _ptr(out))
    return out


def cu_corr_pearson_npn(bed, phen, m, N, p, means, stds):
    bed = np.ascontiguousarray(bed, np.uint8)
    phen = np.ascontiguousarray(phen, np.float32)
    means = np.ascontiguousarray(means, np.float32)
    stds = np.ascontiguousarray(stds, np.float32)
    mxm = np.zeros(max(m * (m - 1) // 2, 1), np.float32)
    mxp = np.zeros(max(m * p, 1), np.float32)
    pxp = np.zeros(max(p * (p - 1) // 2, 1), np.float32)
    lib().cu_corr_pearson_npn(_ptr(bed), _ptr(phen), m, N, p, _ptr(means), _ptr(stds), _ptr(mxm), _ptr(mxp), _ptr(pxp))
    return mxm[: m * (m - 1) // 2], mxp[: m * p], pxp[: p * (p - 1) // 2]


def _strings(v):
    """a sequence of names as the `const char *const *` the writers take"""
    return (C.c_char_p * len(v))(*[str(x).encode() for x in v])


def sumstats_write(outdir: str, mxm_tri, mxp, pxp, chr_ids, snp_ids, ref_alleles, trait_names) -> None:
    """cusk_sumstats_write (host only): <outdir>/mxm.bin, mxp.txt, pxp.txt from arrays -- mxm_tri the lower triangle
    with diagonal of the selected markers' LD, mxp m_total x p for every marker of the .bim, pxp p x p"""
    tri = np.ascontiguousarray(mxm_tri, np.float32).reshape(-1)
    pxp = np.ascontiguousarray(pxp, np.float32)
    p = pxp.shape[0]
    mxp = np.ascontiguousarray(mxp, np.float32).reshape(-1, p)
    m_total = mxp.shape[0]
    k = int((np.sqrt(8.0 * tri.size + 1.0) - 1.0) / 2.0)
    if k * (k + 1) // 2 != tri.size or pxp.shape != (p, p):
        raise ValueError("mxm_tri must hold k (k + 1) / 2 values and pxp must be square")
    if not (len(chr_ids) == len(snp_ids) == len(ref_alleles) == m_total) or len(trait_names) != p:
        raise ValueError("one chr / snp / ref entry per mxp row and one name per trait are needed")

    err = C.create_string_buffer(512)
    rc = lib().cusk_sumstats_write(str(outdir).encode(), _ptr(tri), k, _ptr(mxp), m_total, p, _ptr(pxp), _strings(chr_ids),
                                   _strings(snp_ids), _strings(ref_alleles), _strings(trait_names), err, len(err))
    if rc != 0:
        raise RuntimeError(f"cusk_sumstats_write failed ({rc}): {err.value.decode()}")


def ess_from_se(r: float, se: float) -> float:
    """cusk_ess_from_se: the sample size the mxp / pxp loaders make of a correlation and its standard error"""
    return float(lib().cusk_ess_from_se(float(np.float32(r)), float(np.float32(se))))


def se_from_count(r: float, count: int) -> float:
    """cusk_se_from_count: the standard error written for a Pearson correlation on `count` complete observations, chosen
    so that int(ess_from_se(r, se)) == count"""
    return float(lib().cusk_se_from_count(float(np.float32(r)), int(count)))


def hanning_weights(window: int) -> np.ndarray:
    """cusk_hanning_weights (host only): the window weights `mps block` smooths with, single-precision cosine"""
    out = np.zeros(max(int(window), 1), np.float64)
    if lib().cusk_hanning_weights(int(window), _ptr(out)) != 0:
        raise ValueError(f"cusk_hanning_weights: bad window {window}")
    return out[: int(window)]


def prune_write(bfiles: str, out_stem: str, status) -> None:
    """cusk_prune_write (host only): <out_stem>.bed/.bim/.fam without the markers whose status (one byte per line of
    <bfiles>.bim, as `Engine.ld_prune` gives them per chromosome) is not 0, and <out_stem>.prune.in / .prune.out"""
    status = np.ascontiguousarray(status, np.uint8)
    rc = lib().cusk_prune_write(str(bfiles).encode(), str(out_stem).encode(), _ptr(status), status.size)
    if rc != 0:
        raise RuntimeError(f"cusk_prune_write failed ({rc}): see stderr")


def phen_table_load(table_path: str, fam_path: str | None = None):
    """cusk_phen_table_load (host only) -> (names, data cols x N float32 trait-major, info): a trait or covariate table,
    matched by IID to the individuals of `fam_path` in its order (absent individuals NaN, rows the .fam does not list
    dropped), or with its rows as they come.  info: matched, dropped, in_order.  Raises ValueError with the loader's message
    (line and column of a bad token, a duplicate IID, a ragged row, a header without FID / IID)."""
    h, err = C.c_void_p(), C.create_string_buffer(1024)
    rc = lib().cusk_phen_table_load(C.byref(h), str(table_path).encode(), str(fam_path).encode() if fam_path is not None else None,
                                    err, len(err))
    if rc != 0:
        raise ValueError(err.value.decode())
    try:
        L = lib()
        N, p = int(L.cusk_phen_table_rows(h)), int(L.cusk_phen_table_cols(h))
        names = [L.cusk_phen_table_name(h, j).decode() for j in range(p)]
        data = np.empty((p, N), np.float32)
        if data.size:
            C.memmove(_ptr(data), L.cusk_phen_table_data(h), data.nbytes)
        info = {"matched": int(L.cusk_phen_table_matched(h)), "dropped": int(L.cusk_phen_table_dropped(h)),
                "in_order": bool(L.cusk_phen_table_in_order(h))}
    finally:
        lib().cusk_phen_table_free(h)
    return names, data, info


def phen_write(path: str, fam_path: str, names, data) -> None:
    """cusk_phen_write (host only): a .phen for the individuals of `fam_path` in its order; data p x N float32 trait-major,
    NaN goes out as NA"""
    data = np.ascontiguousarray(data, np.float32)
    if data.ndim != 2 or data.shape[0] != len(names):
        raise ValueError("data must be len(names) x N")
    arr = (C.c_char_p * len(names))(*[str(s).encode() for s in names])
    err = C.create_string_buffer(1024)
    rc = lib().cusk_phen_write(str(path).encode(), str(fam_path).encode(), arr, len(names), _ptr(data), data.shape[1], err, len(err))
    if rc != 0:
        raise RuntimeError(f"cusk_phen_write failed ({rc}): {err.value.decode()}")


def sumstats_write_se(outdir: str, mxp, mxp_n, pxp, pxp_n, chr_ids, snp_ids, ref_alleles, trait_names) -> None:
    """cusk_sumstats_write_se (host only): <outdir>/mxp_se.txt, pxp_se.txt from the correlations sumstats_write wrote and
    the per-pair observation counts of Engine.pair_counts (mxp_n m_total x p, pxp_n p x p)"""
    pxp = np.ascontiguousarray(pxp, np.float32)
    p = pxp.shape[0]
    mxp = np.ascontiguousarray(mxp, np.float32).reshape(-1, p)
    m_total = mxp.shape[0]
    mxp_n = np.ascontiguousarray(mxp_n, np.int32).reshape(-1, p)
    pxp_n = np.ascontiguousarray(pxp_n, np.int32)
    if pxp.shape != (p, p) or pxp_n.shape != (p, p) or mxp_n.shape != mxp.shape:
        raise ValueError("pxp and pxp_n must be p x p, mxp and mxp_n m_total x p")
    if not (len(chr_ids) == len(snp_ids) == len(ref_alleles) == m_total) or len(trait_names) != p:
        raise ValueError("one chr / snp / ref entry per mxp row and one name per trait are needed")

    err = C.create_string_buffer(512)
    rc = lib().cusk_sumstats_write_se(str(outdir).encode(), _ptr(mxp), _ptr(mxp_n), m_total, p, _ptr(pxp), _ptr(pxp_n),
                                      _strings(chr_ids), _strings(snp_ids), _strings(ref_alleles), _strings(trait_names), err, len(err))
    if rc != 0:
        raise RuntimeError(f"cusk_sumstats_write_se failed ({rc}): {err.value.decode()}")


def sumstats_write_se_values(outdir: str, mxp_se, pxp_se, chr_ids, snp_ids, ref_alleles, trait_names) -> None:
    """cusk_sumstats_write_se_values (host only): <outdir>/mxp_se.txt, pxp_se.txt from finished standard errors (mxp_se
    m_total x p, pxp_se p x p with NaN on its diagonal), as `sumstats --ordinal` writes them"""
    pxp_se = np.ascontiguousarray(pxp_se, np.float32)
    p = pxp_se.shape[0]
    mxp_se = np.ascontiguousarray(mxp_se, np.float32).reshape(-1, p)
    m_total = mxp_se.shape[0]
    if pxp_se.shape != (p, p):
        raise ValueError("pxp_se must be p x p, mxp_se m_total x p")
    if not (len(chr_ids) == len(snp_ids) == len(ref_alleles) == m_total) or len(trait_names) != p:
        raise ValueError("one chr / snp / ref entry per mxp row and one name per trait are needed")

    err = C.create_string_buffer(512)
    rc = lib().cusk_sumstats_write_se_values(str(outdir).encode(), _ptr(mxp_se), m_total, p, _ptr(pxp_se), _strings(chr_ids),
                                             _strings(snp_ids), _strings(ref_alleles), _strings(trait_names), err, len(err))
    if rc != 0:
        raise RuntimeError(f"cusk_sumstats_write_se_values failed ({rc}): {err.value.decode()}")


def ordinal_levels(phen, ord_ix):
    """levels (q x 8 float32, ascending, unused ones 0) and their numbers (q int32) of the ordinal traits `ord_ix` (rows of
    phen, p x N): the sorted distinct non-NaN values, as `sumstats --ordinal` takes them"""
    phen = np.asarray(phen, np.float32)
    levels, nlev = np.zeros((len(ord_ix), 8), np.float32), np.zeros(len(ord_ix), np.int32)
    for t, ix in enumerate(ord_ix):
        v = np.unique(phen[ix][~np.isnan(phen[ix])])
        if not 1 <= len(v) <= 8:
            raise ValueError(f"trait {ix} has {len(v)} distinct values; an ordinal trait has 1 to 8")
        levels[t, :len(v)], nlev[t] = v, len(v)
    return levels, nlev


@dataclass
class Stats:
    level: int
    levels_run: int
    max_degree: list
    edges: list
    tests: list
    subsets: list
    removed: list
    kernel_ms: list
    level_ms: list
    total_ms: float
    rechecks: list
    violations: int
    exact_fallbacks: int
    main_kernel_ms: list
    canonical_tests: list

    @staticmethod
    def of(s: CuskStats) -> "Stats":
        return Stats(s.level, s.levels_run, list(s.max_degree), list(s.edges), list(s.tests), list(s.subsets),
                     list(s.removed), list(s.kernel_ms), list(s.level_ms), float(s.total_ms), list(s.rechecks),
                     int(s.violations), int(s.exact_fallbacks), list(s.main_kernel_ms), list(s.canonical_tests))


class DeviceArray:
    """n-byte HBM allocation owned by the library (no torch needed)."""

    def __init__(self, host: np.ndarray | None = None, nbytes: int | None = None):
        self.nbytes = int(host.nbytes if host is not None else nbytes)
        self.ptr = lib().cusk_dev_alloc(self.nbytes)
        if not self.ptr:
            raise MemoryError(f"cusk_dev_alloc({self.nbytes}) failed")
        if host is not None:
            h = np.ascontiguousarray(host)
            if lib().cusk_dev_upload(self.ptr, _ptr(h), h.nbytes) != 0:
                raise RuntimeError("upload failed")

    def download(self, dtype, shape) -> np.ndarray:
        out = np.empty(shape, dtype)
        if lib().cusk_dev_download(_ptr(out), self.ptr, out.nbytes) != 0:
            raise RuntimeError("download failed")
        return out

    def free(self):
        if self.ptr:
            lib().cusk_dev_free(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Engine:
    """Device-resident engine (cusk_engine_* of include/cusk_hip.h)."""

    def __init__(self, device: int = 0, stream: int | None = None):
        h = C.c_void_p()
        rc = lib().cusk_engine_create(C.byref(h), int(device), C.c_void_p(stream) if stream else None)
        if rc != 0:
            raise RuntimeError(f"cusk_engine_create failed with code {rc} (no MI355X / HIP device?)")
        self.h = h

    def close(self):
        if self.h:
            lib().cusk_engine_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != 0:
            raise RuntimeError(f"libcusk_hip error {rc}: {lib().cusk_last_error(self.h).decode()}")

    def set_option(self, key: str, value: int) -> None:
        self._check(lib().cusk_engine_set_option(self.h, key.encode(), int(value)))

    def level1_form(self) -> int:
        """cusk_engine_level1_form: the kernel that ran level 1 in the last run -- 0 generic sweep, 1 pair kernel, 2 / 3 row
        kernel with the row in LDS at 256 / 512 threads, 4 row kernel in its gather form, -1 no level 1 ran"""
        return int(lib().cusk_engine_level1_form(self.h))

    def set_row_shard(self, rank: int, world: int, exchange=None, host_staging: bool = True) -> None:
        """Row-sharded sweep of one block over `world` engines (cusk_engine_set_row_shard).  `exchange(level, buf,
        count, elem_bytes, on_device, stream) -> int` must all-reduce the buffer with an element-wise unsigned MIN
        (see ci-gwas_amd/shard.py: make_min_exchange)."""
        from ._lib import EXCHANGE_FN

        if exchange is None:
            self._exchange_cb = None
            self._check(lib().cusk_engine_set_row_shard(self.h, 0, 1, None, None, 0))
            return

        def trampoline(_user, level, buf, count, elem_bytes, on_device, stream):
            try:
                return int(exchange(int(level), int(buf), int(count), int(elem_bytes), bool(on_device), stream))
            except Exception as exc:  # an exception must not unwind through the C frames
                import traceback

                traceback.print_exc()
                self._exchange_error = exc
                return 1

        self._exchange_cb = EXCHANGE_FN(trampoline)  # keep the thunk alive as long as the engine uses it
        self._check(lib().cusk_engine_set_row_shard(self.h, int(rank), int(world),
                                                    C.cast(self._exchange_cb, C.c_void_p), None, 1 if host_staging else 0))

    @property
    def stream(self) -> int:
        return int(lib().cusk_engine_stream(self.h) or 0)

    def run_skeleton(self, C_dev: int, n: int, Th, maxlevel: int) -> Stats:
        Th = np.ascontiguousarray(Th, np.float32)
        st = CuskStats()
        self._check(lib().cusk_run_skeleton(self.h, C_dev, n, _ptr(Th), int(maxlevel), C.byref(st)))
        return Stats.of(st)

    def run_skeleton_batch(self, C_dev: int, n: int, lo, hi, Th, maxlevel: int) -> Stats:
        """cusk_run_skeleton_batch: blocks [lo[b], hi[b]) on the diagonal of one n x n allocation, swept in one run"""
        Th = np.ascontiguousarray(Th, np.float32)
        lo = np.ascontiguousarray(lo, np.int32)
        hi = np.ascontiguousarray(hi, np.int32)
        st = CuskStats()
        self._check(lib().cusk_run_skeleton_batch(self.h, C_dev, int(n), len(lo), _ptr(lo), _ptr(hi), _ptr(Th), int(maxlevel),
                                                  C.byref(st)))
        self._batch = (lo.copy(), hi.copy())
        return Stats.of(st)

    def run_skeleton_batch_het(self, C_dev: int, N_dev: int, n: int, lo, hi, th: float, maxlevel: int) -> Stats:
        """cusk_run_skeleton_batch_het: the batched run with every test decided at the per-pair sample sizes N_dev (an n x n
        float32 allocation like C_dev with every block's sizes on the diagonal, e.g. from `ess_square_batch`);
        th = hetcor_threshold(alpha).  Results as run_skeleton_batch: adjacency_blocks, sepsets"""
        lo = np.ascontiguousarray(lo, np.int32)
        hi = np.ascontiguousarray(hi, np.int32)
        st = CuskStats()
        self._check(lib().cusk_run_skeleton_batch_het(self.h, C_dev, N_dev, int(n), len(lo), _ptr(lo), _ptr(hi),
                                                      float(np.float32(th)), int(maxlevel), C.byref(st)))
        self._batch = (lo.copy(), hi.copy())
        return Stats.of(st)

    def adjacency_blocks(self) -> list:
        """per block of the last batched run its k x k int32 adjacency (cusk_result_adj_bits_blocks)"""
        lo, hi = self._batch
        k = (hi - lo).astype(np.int64)
        wb = (k + 63) // 64
        out = np.zeros(int((k * wb).sum()), np.uint64)
        self._check(lib().cusk_result_adj_bits_blocks(self.h, _ptr(out)))
        res, o = [], 0
        for kb, w in zip(k, wb):
            bits = out[o:o + kb * w].reshape(kb, w)
            o += kb * w
            G = np.unpackbits(bits.view(np.uint8), axis=1, bitorder="little")[:, :kb].astype(np.int32)
            res.append(G)
        return res

    def gather_rows(self, M_dev: int, n: int, idx, row_src, row_k, row_first, row_out, out_dev: int | None = None,
                    out_count: int = 0):
        idx = np.ascontiguousarray(idx, np.int32)
        row_src = np.ascontiguousarray(row_src, np.int32)
        row_k = np.ascontiguousarray(row_k, np.int32)
        row_first = np.ascontiguousarray(row_first, np.int64)
        row_out = np.ascontiguousarray(row_out, np.int64)
        host = None if out_dev is not None else np.zeros(int(out_count), np.float32)
        self._check(lib().cusk_gather_rows(self.h, M_dev, int(n), _ptr(idx), len(idx), _ptr(row_src), _ptr(row_k), _ptr(row_first),
                                           _ptr(row_out), len(row_src), out_dev if out_dev is not None else _ptr(host),
                                           int(out_count), 1 if out_dev is not None else 0))
        return host

    def run_hetcor(self, C_dev: int, n: int, th: float, maxlevel: int, N_dev: int | None = None,
                   ess_uniform: float = 0.0, G_init_dev: int | None = None, time_index=None) -> Stats:
        ti = np.ascontiguousarray(time_index, np.int32) if time_index is not None else None
        st = CuskStats()
        self._check(lib().cusk_run_hetcor(self.h, C_dev, N_dev, float(ess_uniform), G_init_dev, n,
                                          float(np.float32(th)), int(maxlevel), _ptr(ti), C.byref(st)))
        return Stats.of(st)

    def run_skeleton_het(self, C_dev: int, N_dev: int, n: int, th: float, maxlevel: int) -> Stats:
        """cusk_run_skeleton_het: Skeleton's outputs (adjacency, separating sets, pMax) with every test decided at the
        per-pair sample sizes N_dev (n x n float32 on the device, e.g. from `ess_square`); th = hetcor_threshold(alpha)"""
        st = CuskStats()
        self._check(lib().cusk_run_skeleton_het(self.h, C_dev, N_dev, int(n), float(np.float32(th)), int(maxlevel), C.byref(st)))
        return Stats.of(st)

    def ess_square(self, mxp_ess, pxp_ess, m: int, p: int, n_uniform: float, N_dev: int) -> None:
        """cusk_ess_square: the (m + p)^2 float32 sample-size matrix at the device address N_dev (any float boundary):
        n_uniform between markers, mxp_ess (m x p) mirrored, pxp_ess (p x p) with NaN on its diagonal"""
        mxp_ess = np.ascontiguousarray(mxp_ess, np.float32).reshape(-1) if int(m) * int(p) else None
        pxp_ess = np.ascontiguousarray(pxp_ess, np.float32).reshape(-1) if int(p) else None
        if (mxp_ess is not None and mxp_ess.size != int(m) * int(p)) or (pxp_ess is not None and pxp_ess.size != int(p) * int(p)):
            raise ValueError("ess_square: mxp_ess must hold m * p values and pxp_ess p * p")
        self._check(lib().cusk_ess_square(self.h, _ptr(mxp_ess), _ptr(pxp_ess), int(m), int(p), float(np.float32(n_uniform)), N_dev))

    def ess_square_batch(self, mxp_ess, pxp_ess, m, base, p: int, n_uniform: float, n: int, N_dev: int) -> None:
        """cusk_ess_square_batch: `ess_square` for the blocks of a batch in one launch.  Block b = variables base[b] ..
        base[b] + m[b] + p of the n x n allocation at N_dev (16-byte aligned); mxp_ess = the blocks' m[b] x p tables back
        to back, pxp_ess = one p x p table per block.  Cells outside the diagonal blocks are not written"""
        m = np.ascontiguousarray(m, np.int32)
        base = np.ascontiguousarray(base, np.int32)
        if m.shape != base.shape or m.ndim != 1:
            raise ValueError("ess_square_batch: one marker count and one base per block")
        mxp_ess = np.ascontiguousarray(mxp_ess, np.float32).reshape(-1) if int(m.sum()) * int(p) else None
        pxp_ess = np.ascontiguousarray(pxp_ess, np.float32).reshape(-1) if int(p) else None
        if (mxp_ess is not None and mxp_ess.size != int(m.sum()) * int(p)) or \
                (pxp_ess is not None and pxp_ess.size != len(m) * int(p) * int(p)):
            raise ValueError("ess_square_batch: mxp_ess must hold sum(m) * p values and pxp_ess p * p per block")
        self._check(lib().cusk_ess_square_batch(self.h, _ptr(mxp_ess), _ptr(pxp_ess), len(m), _ptr(m), _ptr(base), int(p),
                                                float(np.float32(n_uniform)), int(n), N_dev))

    def adjacency(self) -> np.ndarray:
        n = lib().cusk_result_n(self.h)
        G = np.zeros((n, n), np.int32)
        self._check(lib().cusk_result_adj_i32(self.h, _ptr(G)))
        return G

    def adjacency_bits(self) -> np.ndarray:
        n, w = lib().cusk_result_n(self.h), lib().cusk_result_words(self.h)
        out = np.zeros((n, w), np.uint64)
        self._check(lib().cusk_dev_download(_ptr(out), lib().cusk_result_adj_bits_dev(self.h), out.nbytes))
        return out

    def pmax(self, C_dev: int) -> np.ndarray:
        n = lib().cusk_result_n(self.h)
        out = np.zeros((n, n), np.float32)
        self._check(lib().cusk_result_pmax(self.h, C_dev, _ptr(out)))
        return out

    def sepsets(self):
        """-> (x, y, level, z, S[count,14]) sparse records, sorted by (x, y)."""
        cnt = lib().cusk_result_sepsets(self.h, None, None, None, None, None)
        if cnt < 0:
            raise RuntimeError("no Skeleton result")
        x, y, lv = (np.zeros(cnt, np.int32) for _ in range(3))
        z = np.zeros(cnt, np.float32)
        S = np.full((cnt, ML), -1, np.int32)
        if cnt:
            lib().cusk_result_sepsets(self.h, _ptr(x), _ptr(y), _ptr(lv), _ptr(z), _ptr(S))
            o = np.lexsort((y, x))
            x, y, lv, z, S = x[o], y[o], lv[o], z[o], S[o]
        return x, y, lv, z, S

    def corr_build(self, bed, phen, m, N, p, means, stds, C_dev: int, want_mxp: bool = False):
        bed = np.ascontiguousarray(bed, np.uint8)
        phen = np.ascontiguousarray(phen, np.float32)
        means = np.ascontiguousarray(means, np.float32)
        stds = np.ascontiguousarray(stds, np.float32)
        mxp = np.zeros(m * p, np.float32) if want_mxp else None
        self._check(lib().cusk_corr_build(self.h, _ptr(bed), _ptr(phen), m, N, p, _ptr(means), _ptr(stds), C_dev, _ptr(mxp)))
        return mxp

    def corr_build_indexed(self, bed, phen, marker_ix, m_total: int, N: int, p: int, means, stds, C_dev: int,
                           want_mxp: bool = False):
        """cusk_corr_build_indexed: the build of the markers `marker_ix` (ascending global indices) of a .bed of m_total
        markers.  bed / means / stds: host arrays of ALL markers, or DeviceArray copies of them (then the rows are
        gathered on the device); the matrix in C_dev has the selected markers in index order, then the traits"""
        def arg(a, dtype):
            if isinstance(a, DeviceArray):
                return a, a.ptr
            a = np.ascontiguousarray(a, dtype)
            return a, _ptr(a)

        bed, bed_p = arg(bed, np.uint8)
        means, means_p = arg(means, np.float32)
        stds, stds_p = arg(stds, np.float32)
        phen = np.ascontiguousarray(phen, np.float32)
        ix = np.ascontiguousarray(marker_ix, np.int32)
        mxp = np.zeros(len(ix) * p, np.float32) if want_mxp else None
        self._check(lib().cusk_corr_build_indexed(self.h, bed_p, _ptr(phen), _ptr(ix), len(ix), int(m_total), int(N), int(p),
                                                  means_p, stds_p, C_dev, _ptr(mxp)))
        return mxp

    def pair_counts(self, bed, phen, N: int, p: int, k: int | None = None, marker_ix=None, m_total: int | None = None):
        """cusk_pair_counts -> (mxp_n k x p, pxp_n p x p) int32: per pair the individuals with both values observed (marker
        not missing, trait not NaN).  bed / phen: host arrays or DeviceArray copies; the markers are rows `marker_ix`
        (ascending) of the m_total rows of bed, or its first k rows (default: all rows of a host array)"""
        clb = (int(N) + 3) // 4
        if isinstance(bed, DeviceArray):
            bed_p, rows = bed.ptr, bed.nbytes // clb
        else:
            bed = np.ascontiguousarray(bed, np.uint8)
            bed_p, rows = _ptr(bed), bed.size // clb
        if isinstance(phen, DeviceArray):
            phen_p = phen.ptr
        else:
            phen = np.ascontiguousarray(phen, np.float32)
            phen_p = _ptr(phen)
        m_total = int(rows if m_total is None else m_total)
        ix = np.ascontiguousarray(marker_ix, np.int32) if marker_ix is not None else None
        k = int(len(ix) if ix is not None else (m_total if k is None else k))
        mxp_n, pxp_n = np.zeros((k, int(p)), np.int32), np.zeros((int(p), int(p)), np.int32)
        self._check(lib().cusk_pair_counts(self.h, bed_p, phen_p, _ptr(ix), k, m_total, int(N), int(p), _ptr(mxp_n), _ptr(pxp_n)))
        return mxp_n, pxp_n

    def phen_moments(self, phen, N: int, p: int):
        """cusk_phen_moments -> (n int32, mean, sd float64) per trait over its finite values (population sd); phen p x N
        trait-major, a host array or a DeviceArray"""
        if isinstance(phen, DeviceArray):
            phen_p = phen.ptr
        else:
            phen = np.ascontiguousarray(phen, np.float32)
            phen_p = _ptr(phen)
        n, mean, sd = np.zeros(int(p), np.int32), np.zeros(int(p)), np.zeros(int(p))
        self._check(lib().cusk_phen_moments(self.h, phen_p, int(N), int(p), _ptr(n), _ptr(mean), _ptr(sd)))
        return n, mean, sd

    def phen_adjust(self, phen, covar, N: int, p: int, c: int, adjust=None, out=None, stats=None):
        """cusk_phen_adjust -> dict(out p x N float32, n, mean, sd, beta p x (c + 1), r2, status): every trait residualised
        on the c covariates (where adjust[t], default all) and standardised to mean 0 and population sd 1 over its observed
        values; the rule is stated in include/cusk_hip.h.  phen p x N and covar c x N float32, NaN = missing, host arrays
        or DeviceArray copies.  `out` (p * N float32 at its start) and `stats` (dict of preallocated n / mean / sd / beta /
        r2 / status arrays) let a caller put guards behind the results."""
        N, p, c = int(N), int(p), int(c)
        if isinstance(phen, DeviceArray):
            phen_p = phen.ptr
        else:
            phen = np.ascontiguousarray(phen, np.float32)
            phen_p = _ptr(phen)
        if covar is None:
            covar_p = None
        elif isinstance(covar, DeviceArray):
            covar_p = covar.ptr
        else:
            covar = np.ascontiguousarray(covar, np.float32)
            covar_p = _ptr(covar)
        adjust = np.ones(p, np.uint8) if adjust is None else np.ascontiguousarray(adjust, np.uint8)
        if adjust.size != p:
            raise ValueError("one adjust flag per trait is needed")
        stats = dict(stats or {})
        res = {"out": np.empty(p * N, np.float32) if out is None else out,
               "n": stats.get("n", np.zeros(p, np.int32)), "mean": stats.get("mean", np.zeros(p)), "sd": stats.get("sd", np.zeros(p)),
               "beta": stats.get("beta", np.zeros(p * (c + 1))), "r2": stats.get("r2", np.zeros(p)),
               "status": stats.get("status", np.zeros(p, np.int32))}
        self._check(lib().cusk_phen_adjust(self.h, phen_p, covar_p, N, p, c, _ptr(adjust), _ptr(res["out"]), _ptr(res["n"]),
                                           _ptr(res["mean"]), _ptr(res["sd"]), _ptr(res["beta"]), _ptr(res["r2"]), _ptr(res["status"])))
        res["out"] = res["out"][:p * N].reshape(p, N)
        res["beta"] = res["beta"][:p * (c + 1)].reshape(p, c + 1)
        for key in ("n", "mean", "sd", "r2", "status"):
            res[key] = res[key][:p]
        return res

    def phen_timing(self):
        """cusk_phen_timing: ms of scaling, Gram, solve, moments, standardise in the last phen_adjust"""
        ms = np.zeros(5, np.float32)
        lib().cusk_phen_timing(self.h, _ptr(ms))
        return ms

    def phen_rint(self, vals, N: int, p: int, select=None, offset: float = 0.375, out=None, stats=None, ranks: bool = False):
        """cusk_phen_rint -> dict(out p x N float32, n, mean, sd, status[, rank2 p x N uint32]): the rank-based inverse normal
        transform of the selected traits (default all): average ranks over the finite values, normal scores of
        (rank - offset) / (n + 1 - 2 offset), standardised to mean 0 and population sd 1; the rule is stated in
        include/cusk_hip.h.  vals p x N float32, NaN / Inf = missing, a host array or a DeviceArray.  A trait that is not
        selected passes through.  `out` (p * N float32 at its start) and `stats` (dict of preallocated n / mean / sd / status /
        rank2 arrays) let a caller put guards behind the results; ranks=True also returns rank2 = twice the average rank."""
        N, p = int(N), int(p)
        if isinstance(vals, DeviceArray):
            vals_p = vals.ptr
        else:
            vals = np.ascontiguousarray(vals, np.float32)
            vals_p = _ptr(vals)
        if select is not None:
            select = np.ascontiguousarray(select, np.uint8)
            if select.size != p:
                raise ValueError("one select flag per trait is needed")
        stats = dict(stats or {})
        res = {"out": np.empty(p * N, np.float32) if out is None else out,
               "n": stats.get("n", np.zeros(p, np.int32)), "mean": stats.get("mean", np.zeros(p)), "sd": stats.get("sd", np.zeros(p)),
               "status": stats.get("status", np.zeros(p, np.int32))}
        if ranks or "rank2" in stats:
            res["rank2"] = stats.get("rank2", np.zeros(p * N, np.uint32))
        self._check(lib().cusk_phen_rint(self.h, vals_p, N, p, _ptr(select), float(offset), _ptr(res["out"]), _ptr(res["n"]),
                                         _ptr(res["mean"]), _ptr(res["sd"]), _ptr(res["status"]), _ptr(res.get("rank2"))))
        res["out"] = res["out"][:p * N].reshape(p, N)
        if "rank2" in res:
            res["rank2"] = res["rank2"][:p * N].reshape(p, N)
        for key in ("n", "mean", "sd", "status"):
            res[key] = res[key][:p]
        return res

    def phen_rint_timing(self):
        """cusk_phen_rint_timing: ms of keys, sort, ranks, moments + standardise in the last phen_rint"""
        ms = np.zeros(4, np.float32)
        lib().cusk_phen_rint_timing(self.h, _ptr(ms))
        return ms

    def ordinal_tables(self, bed, phen, N: int, p: int, ord_ix, levels, nlev, k: int | None = None, marker_ix=None,
                       m_total: int | None = None, want_mxo: bool = True):
        """cusk_ordinal_tables -> (mxo k x q x 3 x 8, oxo q x q x 8 x 8) int32 contingency tables of the ordinal traits
        `ord_ix` (rows of phen) with the genotype classes of the markers and with one another; levels / nlev as
        `ordinal_levels` gives them.  bed / phen, k, marker_ix, m_total as `pair_counts` takes them; want_mxo=False
        counts the trait tables only (bed may then be None)"""
        clb = (int(N) + 3) // 4
        ord_ix = np.ascontiguousarray(ord_ix, np.int32)
        levels = np.ascontiguousarray(levels, np.float32).reshape(len(ord_ix), 8)
        nlev = np.ascontiguousarray(nlev, np.int32)
        q = len(ord_ix)
        if isinstance(phen, DeviceArray):
            phen_p = phen.ptr
        else:
            phen = np.ascontiguousarray(phen, np.float32)
            phen_p = _ptr(phen)
        mxo, ix, bed_p = None, None, None
        if want_mxo:
            if isinstance(bed, DeviceArray):
                bed_p, rows = bed.ptr, bed.nbytes // clb
            else:
                bed = np.ascontiguousarray(bed, np.uint8)
                bed_p, rows = _ptr(bed), bed.size // clb
            m_total = int(rows if m_total is None else m_total)
            ix = np.ascontiguousarray(marker_ix, np.int32) if marker_ix is not None else None
            k = int(len(ix) if ix is not None else (m_total if k is None else k))
            mxo = np.zeros((k, q, 3, 8), np.int32)
        else:
            k, m_total = 0, 0
        oxo = np.zeros((q, q, 8, 8), np.int32)
        self._check(lib().cusk_ordinal_tables(self.h, bed_p, phen_p, _ptr(ix), k, m_total, int(N), int(p), _ptr(ord_ix), q,
                                              _ptr(levels), _ptr(nlev), _ptr(mxo), _ptr(oxo)))
        return mxo, oxo

    def polychoric_fit(self, tables, ka: int | None = None, kb: int | None = None, ntab: int | None = None):
        """cusk_polychoric_fit -> (r float64, se float64, status int32), one entry per table.  tables: an int32 array whose
        last two axes are a table (ka x kb, at most 8 x 8), or a DeviceArray with ka, kb and ntab given.  status: 0 fitted,
        1 boundary (se NaN), 2 degenerate (r and se NaN)"""
        if isinstance(tables, DeviceArray):
            tab_p, shape = tables.ptr, (int(ntab),)
        else:
            tables = np.ascontiguousarray(tables, np.int32)
            ka, kb = tables.shape[-2:]
            shape = tables.shape[:-2]
            ntab, tab_p = int(np.prod(shape, dtype=np.int64)), _ptr(tables)
        r, se, status = np.zeros(ntab, np.float64), np.zeros(ntab, np.float64), np.zeros(ntab, np.int32)
        self._check(lib().cusk_polychoric_fit(self.h, tab_p, int(ntab), int(ka), int(kb), _ptr(r), _ptr(se), _ptr(status)))
        return r.reshape(shape), se.reshape(shape), status.reshape(shape)

    def polyserial_fit(self, phen, N: int, p: int, cont_ix, ord_ix, levels, nlev):
        """cusk_polyserial_fit -> (r, se, status), each len(cont_ix) x len(ord_ix): the two-step polyserial correlation of
        every continuous trait `cont_ix` with every ordinal trait `ord_ix` (rows of phen, host array or DeviceArray) on
        the pair's complete observations"""
        cont_ix = np.ascontiguousarray(cont_ix, np.int32)
        ord_ix = np.ascontiguousarray(ord_ix, np.int32)
        levels = np.ascontiguousarray(levels, np.float32).reshape(len(ord_ix), 8)
        nlev = np.ascontiguousarray(nlev, np.int32)
        if isinstance(phen, DeviceArray):
            phen_p = phen.ptr
        else:
            phen = np.ascontiguousarray(phen, np.float32)
            phen_p = _ptr(phen)
        shape = (len(cont_ix), len(ord_ix))
        r, se, status = np.zeros(shape, np.float64), np.zeros(shape, np.float64), np.zeros(shape, np.int32)
        self._check(lib().cusk_polyserial_fit(self.h, phen_p, int(N), int(p), _ptr(cont_ix), len(cont_ix), _ptr(ord_ix),
                                              len(ord_ix), _ptr(levels), _ptr(nlev), _ptr(r), _ptr(se), _ptr(status)))
        return r, se, status

    def ordinal_timing(self):
        """cusk_ordinal_timing -> kernel ms of the last ordinal_tables (marker tables), polychoric_fit, polyserial_fit"""
        ms = np.zeros(3, np.float32)
        lib().cusk_ordinal_timing(self.h, _ptr(ms))
        return tuple(float(v) for v in ms)

    def marker_pair_sizes(self, bed, N: int, N_dev: int, ld: int, k: int | None = None, marker_ix=None,
                          m_total: int | None = None) -> None:
        """cusk_marker_pair_sizes: float32 counts of the individuals on which both markers of a pair are not missing, over
        the k x k corner of the device matrix at N_dev (leading dimension ld; call it after `ess_square`).  bed: host array
        or DeviceArray; the markers are rows `marker_ix` (ascending) of its m_total rows, or its first k rows (default: all
        rows of a host array)"""
        clb = (int(N) + 3) // 4
        if isinstance(bed, DeviceArray):
            bed_p, rows = bed.ptr, bed.nbytes // clb
        else:
            bed = np.ascontiguousarray(bed, np.uint8)
            bed_p, rows = _ptr(bed), bed.size // clb
        m_total = int(rows if m_total is None else m_total)
        ix = np.ascontiguousarray(marker_ix, np.int32) if marker_ix is not None else None
        k = int(len(ix) if ix is not None else (m_total if k is None else k))
        self._check(lib().cusk_marker_pair_sizes(self.h, bed_p, _ptr(ix), k, m_total, int(N), N_dev, int(ld)))

    def marker_pair_sizes_batch(self, bed, N: int, m, base, n: int, N_dev: int, marker_ix=None, m_total: int | None = None) -> None:
        """cusk_marker_pair_sizes_batch: `marker_pair_sizes` for the blocks of a batch in one launch.  Block b = m[b] markers
        at the variables base[b] .. of the n x n allocation at N_dev (call it after `ess_square_batch`); marker_ix = the
        .bed rows of all blocks in one list, block after block (a row may repeat; None = rows 0 .. sum(m) - 1)"""
        clb = (int(N) + 3) // 4
        if isinstance(bed, DeviceArray):
            bed_p, rows = bed.ptr, bed.nbytes // clb
        else:
            bed = np.ascontiguousarray(bed, np.uint8)
            bed_p, rows = _ptr(bed), bed.size // clb
        m = np.ascontiguousarray(m, np.int32)
        base = np.ascontiguousarray(base, np.int32)
        if m.shape != base.shape or m.ndim != 1:
            raise ValueError("marker_pair_sizes_batch: one marker count and one base per block")
        ix = np.ascontiguousarray(marker_ix, np.int32) if marker_ix is not None else None
        if ix is not None and ix.size != int(m.sum()):
            raise ValueError("marker_pair_sizes_batch: marker_ix must hold sum(m) rows")
        m_total = int(rows if m_total is None else m_total)
        self._check(lib().cusk_marker_pair_sizes_batch(self.h, bed_p, _ptr(ix), m_total, int(N), len(m), _ptr(m), _ptr(base), int(n),
                                                       N_dev))

    def pack_lower_tri(self, C_dev: int, n: int, k: int) -> np.ndarray:
        """the leading k x k block of the n x n device matrix as the `mxm` file holds it: lower triangle with diagonal,
        row-major, NaN -> 0 (cusk_pack_lower_tri)"""
        out = np.empty(k * (k + 1) // 2, np.float32)
        self._check(lib().cusk_pack_lower_tri(self.h, C_dev, int(n), int(k), _ptr(out), 0))
        return out

    def nan_to_zero(self, M_dev: int, count: int) -> None:
        """NaN -> 0 in place on `count` floats of a device allocation (cusk_nan_to_zero); asynchronous on the engine's
        stream: read the result with `download` or hand it to a run of this engine"""
        self._check(lib().cusk_nan_to_zero(self.h, M_dev, int(count)))

    def download(self, src_dev: int, dtype, shape) -> np.ndarray:
        """device -> host copy ordered after the engine's work (cusk_engine_download)"""
        out = np.empty(shape, dtype)
        self._check(lib().cusk_engine_download(self.h, _ptr(out), src_dev, out.nbytes))
        return out

    def corr_banded(self, bed, m: int, N: int, width: int, want_band: bool = False):
        """`mps block`'s device part for one chromosome: forward row sums of |banded Kendall-npn correlations|
        (and the band itself, m x width, on request)"""
        bed = np.ascontiguousarray(bed, np.uint8)
        sums = np.zeros(m, np.float32)
        band = np.zeros((m, width), np.float32) if want_band else None
        self._check(lib().cusk_corr_banded(self.h, _ptr(bed), m, N, width, _ptr(sums), _ptr(band)))
        return (sums, band) if want_band else sums

    def genotype_counts(self, bed, m: int, N: int, out=None) -> np.ndarray:
        """cusk_genotype_counts: (m, 4) int32, per marker the individuals < N with .bed code 00, 01, 10, 11 (dosage 2,
        missing, dosage 1, dosage 0).  `out` may be given (int32, at least 4 m entries) to be filled in place."""
        bed = np.ascontiguousarray(bed, np.uint8)
        if bed.size < int(m) * ((int(N) + 3) // 4):
            raise ValueError("genotype_counts: bed holds fewer than m rows of ceil(N / 4) bytes")
        out = np.zeros(4 * max(int(m), 1), np.int32) if out is None else out
        assert out.dtype == np.int32 and out.flags.c_contiguous and out.size >= 4 * m
        self._check(lib().cusk_genotype_counts(self.h, _ptr(bed), int(m), int(N), _ptr(out)))
        return out.reshape(-1)[:4 * m].reshape(m, 4)

    def ld_prune_scan(self, conflict_bits, constant_flags, m: int, W: int, out=None) -> np.ndarray:
        """cusk_ld_prune_scan: the greedy pass of `ld_prune` alone on a conflict bitmap (m rows of ceil(W / 64) uint64
        words, bit b of word k of row i = pair (i, i + 1 + 64 k + b)) and one constant flag per marker -> m status bytes
        (0 kept, 1 constant, 2 dropped for LD).  `out` may be given (uint8, at least m entries)."""
        bits = np.ascontiguousarray(conflict_bits, np.uint64)
        flags = np.ascontiguousarray(constant_flags, np.uint8)
        if bits.size != int(m) * ((int(W) + 63) // 64) or flags.size != int(m):
            raise ValueError("ld_prune_scan: m rows of ceil(W / 64) words and m flags")
        out = np.zeros(max(int(m), 1), np.uint8) if out is None else out
        assert out.dtype == np.uint8 and out.flags.c_contiguous and out.size >= m
        self._check(lib().cusk_ld_prune_scan(self.h, _ptr(bits), _ptr(flags), int(m), int(W), _ptr(out)))
        return out[:m]

    def ld_prune(self, bed, m: int, N: int, W: int, r_max: float, want_counts: bool = False):
        """cusk_ld_prune for one chromosome: m status bytes (0 kept, 1 constant, 2 dropped for LD: |r| >= r_max with an
        earlier kept marker within W, r the banded correlation of `corr_banded`); with want_counts also the (m, 4)
        genotype counts.  The first kept marker wins (not PLINK's rule)."""
        bed = np.ascontiguousarray(bed, np.uint8)
        if bed.size < int(m) * ((int(N) + 3) // 4):
            raise ValueError("ld_prune: bed holds fewer than m rows of ceil(N / 4) bytes")
        status = np.zeros(max(int(m), 1), np.uint8)
        counts = np.zeros((max(int(m), 1), 4), np.int32) if want_counts else None
        self._check(lib().cusk_ld_prune(self.h, _ptr(bed), int(m), int(N), int(W), float(r_max), _ptr(status), _ptr(counts)))
        return (status[:m], counts[:m]) if want_counts else status[:m]

    def ld_prune_timing(self) -> dict:
        """device milliseconds of the phases of the last `ld_prune` (cusk_ld_prune_timing)"""
        ms = np.zeros(5, np.float32)
        lib().cusk_ld_prune_timing(self.h, _ptr(ms))
        return dict(zip(("upload", "band", "counts", "bitmap", "scan"), (float(v) for v in ms)))

    def hanning_smooth(self, v, weights, out=None):
        """cusk_hanning_smooth: out[c] = sum_i weights[i] * v[c - window // 2 + i] where the window fits, 0 elsewhere
        (float64, accumulated in window order on the device).  `out` may be given (float64, at least len(v) entries) to
        be filled in place; the first len(v) entries are returned."""
        v = np.ascontiguousarray(v, np.float32)
        weights = np.ascontiguousarray(weights, np.float64)
        n = v.shape[0]
        out = np.zeros(max(n, 1), np.float64) if out is None else out
        assert out.dtype == np.float64 and out.flags.c_contiguous and out.shape[0] >= n
        self._check(lib().cusk_hanning_smooth(self.h, _ptr(v), n, _ptr(weights), weights.shape[0], _ptr(out)))
        return out[:n]

    def block_chr(self, row_sums, max_block_size: int) -> list[tuple[int, int]]:
        """cusk_block_chr, the code of `mps block` for one chromosome: (first, last) chromosome-local marker indices of
        the LD blocks cut from the forward row sums"""
        v = np.ascontiguousarray(row_sums, np.float32)
        n = v.shape[0]
        first = np.zeros(max(n, 1), np.int64)
        last = np.zeros(max(n, 1), np.int64)
        count = C.c_size_t(0)
        self._check(lib().cusk_block_chr(self.h, _ptr(v), n, int(max_block_size), _ptr(first), _ptr(last), n, C.byref(count)))
        return [(int(first[k]), int(last[k])) for k in range(count.value)]

    def sepselect_greedy(self, trait_corr, pair_i, pair_j, pair_corr, cand_off, cand, thr):
        """Batched greedy separating-set selection (sepselect.py:262-329) on the device.  Returns
        (sel, sel_len, flags, kernel_ms); see include/cusk_hip.h for the layouts."""
        trait_corr = np.ascontiguousarray(trait_corr, np.float64)
        n, p = trait_corr.shape
        pair_i = np.ascontiguousarray(pair_i, np.int32)
        pair_j = np.ascontiguousarray(pair_j, np.int32)
        pair_corr = np.ascontiguousarray(pair_corr, np.float64)
        cand_off = np.ascontiguousarray(cand_off, np.int64)
        cand = np.ascontiguousarray(cand, np.int32)
        thr = np.ascontiguousarray(thr, np.float64)
        npairs = pair_i.shape[0]
        assert pair_j.shape[0] == npairs and pair_corr.shape[0] == npairs and cand_off.shape[0] == npairs + 1
        assert cand.shape[0] == int(cand_off[-1])
        sel = np.full(max(cand.shape[0], 1), -1, np.int32)
        sel_len = np.zeros(max(npairs, 1), np.int32)
        flags = np.zeros(max(npairs, 1), np.int32)
        ms = np.zeros(1, np.float32)
        self._check(lib().cusk_sepselect_greedy(self.h, _ptr(trait_corr), n, p, npairs, _ptr(pair_i), _ptr(pair_j),
                                                _ptr(pair_corr), _ptr(cand_off), _ptr(cand), _ptr(thr), thr.shape[0],
                                                _ptr(sel), _ptr(sel_len), _ptr(flags), _ptr(ms)))
        return sel, sel_len[:npairs], flags[:npairs], float(ms[0])

    def sepselect_greedy_het(self, trait_corr, pair_i, pair_j, pair_corr, cand_off, cand, trait_n, pair_n, q):
        """`sepselect_greedy` at per-pair sample sizes (cusk_sepselect_greedy_het): `trait_n` is the n x p int32 table of
        sample sizes in the layout of `trait_corr`, `pair_n` the size of every outer pair, `q` = norm.ppf(1 - alpha / 2)."""
        trait_corr = np.ascontiguousarray(trait_corr, np.float64)
        n, p = trait_corr.shape
        pair_i = np.ascontiguousarray(pair_i, np.int32)
        pair_j = np.ascontiguousarray(pair_j, np.int32)
        pair_corr = np.ascontiguousarray(pair_corr, np.float64)
        cand_off = np.ascontiguousarray(cand_off, np.int64)
        cand = np.ascontiguousarray(cand, np.int32)
        trait_n = np.ascontiguousarray(trait_n, np.int32)
        pair_n = np.ascontiguousarray(pair_n, np.int32)
        npairs = pair_i.shape[0]
        assert trait_n.shape == (n, p) and pair_n.shape[0] == npairs
        assert pair_j.shape[0] == npairs and pair_corr.shape[0] == npairs and cand_off.shape[0] == npairs + 1
        assert cand.shape[0] == int(cand_off[-1])
        sel = np.full(max(cand.shape[0], 1), -1, np.int32)
        sel_len = np.zeros(max(npairs, 1), np.int32)
        flags = np.zeros(max(npairs, 1), np.int32)
        ms = np.zeros(1, np.float32)
        self._check(lib().cusk_sepselect_greedy_het(self.h, _ptr(trait_corr), n, p, npairs, _ptr(pair_i), _ptr(pair_j),
                                                    _ptr(pair_corr), _ptr(cand_off), _ptr(cand), _ptr(trait_n), _ptr(pair_n),
                                                    float(q), _ptr(sel), _ptr(sel_len), _ptr(flags), _ptr(ms)))
        return sel, sel_len[:npairs], flags[:npairs], float(ms[0])

    def _iv_args(self, trait_corr, set_off, sets, item_x, item_y, item_set):
        trait_corr = np.ascontiguousarray(trait_corr, np.float64)
        set_off = np.ascontiguousarray(set_off, np.int32).reshape(-1)
        if set_off.shape[0] == 0:
            set_off = np.zeros(1, np.int32)
        sets = np.ascontiguousarray(sets, np.int32).reshape(-1)
        item_x = np.ascontiguousarray(item_x, np.int32).reshape(-1)
        item_y = np.ascontiguousarray(item_y, np.int32).reshape(-1)
        item_set = np.ascontiguousarray(item_set, np.int32).reshape(-1)
        nitems = item_x.shape[0]
        assert trait_corr.ndim == 2 and item_y.shape[0] == nitems and item_set.shape[0] == nitems
        assert sets.shape[0] >= int(set_off[-1])
        return trait_corr, set_off, sets, item_x, item_y, item_set, nitems

    def iv_check(self, trait_corr, set_off, sets, item_x, item_y, item_set, thr, z=None, flags=None):
        """Batched tests (x, y | S) of the instrument filter (cusk_iv_check): `sets[set_off[s]:set_off[s + 1]]` are the
        trait ids of set s, `item_set` = -1 is the empty set, `thr[l]` the threshold at |S| = l (l = 0 .. p-1).  Returns
        (z float64, flags int32, kernel_ms) in the caller's item order; `z` / `flags` may be given to be filled in place."""
        trait_corr, set_off, sets, item_x, item_y, item_set, nitems = self._iv_args(trait_corr, set_off, sets, item_x, item_y,
                                                                                    item_set)
        n, p = trait_corr.shape
        thr = np.ascontiguousarray(thr, np.float64)
        assert thr.shape[0] >= p
        z = np.zeros(max(nitems, 1), np.float64) if z is None else z
        flags = np.zeros(max(nitems, 1), np.int32) if flags is None else flags
        assert z.dtype == np.float64 and flags.dtype == np.int32 and z.shape[0] >= nitems and flags.shape[0] >= nitems
        ms = np.zeros(1, np.float32)
        self._check(lib().cusk_iv_check(self.h, _ptr(trait_corr), n, p, set_off.shape[0] - 1, _ptr(set_off), _ptr(sets), nitems,
                                        _ptr(item_x), _ptr(item_y), _ptr(item_set), _ptr(thr), _ptr(z), _ptr(flags), _ptr(ms)))
        return z[:nitems], flags[:nitems], float(ms[0])

    def iv_check_het(self, trait_corr, set_off, sets, item_x, item_y, item_set, trait_n, q, z=None, flags=None):
        """`iv_check` at per-pair sample sizes (cusk_iv_check_het): `trait_n` is the n x p int32 table of sample sizes in the
        layout of `trait_corr`, `q` = norm.ppf(1 - alpha / 2)."""
        trait_corr, set_off, sets, item_x, item_y, item_set, nitems = self._iv_args(trait_corr, set_off, sets, item_x, item_y,
                                                                                    item_set)
        n, p = trait_corr.shape
        trait_n = np.ascontiguousarray(trait_n, np.int32)
        assert trait_n.shape == (n, p)
        z = np.zeros(max(nitems, 1), np.float64) if z is None else z
        flags = np.zeros(max(nitems, 1), np.int32) if flags is None else flags
        assert z.dtype == np.float64 and flags.dtype == np.int32 and z.shape[0] >= nitems and flags.shape[0] >= nitems
        ms = np.zeros(1, np.float32)
        self._check(lib().cusk_iv_check_het(self.h, _ptr(trait_corr), n, p, set_off.shape[0] - 1, _ptr(set_off), _ptr(sets),
                                            nitems, _ptr(item_x), _ptr(item_y), _ptr(item_set), _ptr(trait_n), float(q),
                                            _ptr(z), _ptr(flags), _ptr(ms)))
        return z[:nitems], flags[:nitems], float(ms[0])

    @staticmethod
    def _mvivw_args(beta, weight, outcome, iv_off, iv, ex_off, ex, theta, se, stats, status):
        """The arguments `mvivw` and `mvivw_ld` share, as contiguous arrays of the ABI's types, and the four output arrays
        (the caller's, or new ones) -> (beta, weight, outcome, iv_off, iv, ex_off, ex, theta, se, stats, status)"""
        beta = np.ascontiguousarray(beta, np.float64)
        weight = np.ascontiguousarray(weight, np.float64)
        assert beta.ndim == 2 and weight.shape == beta.shape
        outcome = np.ascontiguousarray(outcome, np.int32).reshape(-1)
        iv_off = np.ascontiguousarray(iv_off, np.int64).reshape(-1)
        ex_off = np.ascontiguousarray(ex_off, np.int32).reshape(-1)
        iv = np.ascontiguousarray(iv, np.int32).reshape(-1)
        ex = np.ascontiguousarray(ex, np.int32).reshape(-1)
        nout = outcome.shape[0]
        assert iv_off.shape[0] == nout + 1 and ex_off.shape[0] == nout + 1
        assert iv.shape[0] >= int(iv_off.max()) and ex.shape[0] >= int(ex_off.max())
        nex = max(int(ex_off.max()), 1)
        theta = np.full(nex, np.nan) if theta is None else theta
        se = np.full(nex, np.nan) if se is None else se
        stats = np.full((max(nout, 1), 3), np.nan) if stats is None else stats
        status = np.zeros(max(nout, 1), np.int32) if status is None else status
        assert theta.dtype == np.float64 and se.dtype == np.float64 and stats.dtype == np.float64 and status.dtype == np.int32
        assert theta.shape[0] >= nex and se.shape[0] >= nex and stats.size >= 3 * nout and status.shape[0] >= nout
        assert all(a.flags.c_contiguous for a in (theta, se, stats, status))
        return beta, weight, outcome, iv_off, iv, ex_off, ex, theta, se, stats, status

    def mvivw(self, beta, weight, outcome, iv_off, iv, ex_off, ex, model=0, theta=None, se=None, stats=None, status=None):
        """Multivariable IVW regressions of a batch of outcomes (cusk_mvivw; the rule is stated in include/cusk_hip.h):
        `beta`, `weight` M x p float64, `iv[iv_off[a]:iv_off[a + 1]]` the ascending instrument rows and
        `ex[ex_off[a]:ex_off[a + 1]]` the ascending exposure traits of outcome a.  Returns (theta, se, stats, status,
        kernel_ms): theta and se at the positions of `ex`, stats nout x 3 (rss, sigma, smallest squared pivot).  The four
        output arrays may be given to be filled in place."""
        beta, weight, outcome, iv_off, iv, ex_off, ex, theta, se, stats, status = self._mvivw_args(
            beta, weight, outcome, iv_off, iv, ex_off, ex, theta, se, stats, status)
        (M, p), nout = beta.shape, outcome.shape[0]
        ms = np.zeros(1, np.float32)
        self._check(lib().cusk_mvivw(self.h, _ptr(beta), _ptr(weight), M, p, nout, _ptr(outcome), _ptr(iv_off), _ptr(iv),
                                     _ptr(ex_off), _ptr(ex), int(model), _ptr(theta), _ptr(se), _ptr(stats), _ptr(status),
                                     _ptr(ms)))
        return theta, se, stats.reshape(-1)[:3 * nout].reshape(nout, 3), status[:nout], float(ms[0])

    def mvivw_ld(self, beta, weight, ld, outcome, iv_off, iv, ex_off, ex, model=0, ridge=0.0, theta=None, se=None, stats=None,
                 status=None):
        """`mvivw` with correlated instruments by generalised least squares (cusk_mvivw_ld; the rule is stated in
        include/cusk_hip.h): `ld` M x M float64, of which the strict lower triangle is read, `ridge` in [0, 1).  The other
        arguments and the return value are those of `mvivw`; stats[:, 2] is the smallest squared pivot of the LD matrix
        (status 0) or the pivot that failed (status 4)."""
        beta, weight, outcome, iv_off, iv, ex_off, ex, theta, se, stats, status = self._mvivw_args(
            beta, weight, outcome, iv_off, iv, ex_off, ex, theta, se, stats, status)
        (M, p), nout = beta.shape, outcome.shape[0]
        ld = np.ascontiguousarray(ld, np.float64)
        assert ld.shape == (M, M)
        ms = np.zeros(1, np.float32)
        self._check(lib().cusk_mvivw_ld(self.h, _ptr(beta), _ptr(weight), _ptr(ld), float(ridge), M, p, nout, _ptr(outcome),
                                        _ptr(iv_off), _ptr(iv), _ptr(ex_off), _ptr(ex), int(model), _ptr(theta), _ptr(se),
                                        _ptr(stats), _ptr(status), _ptr(ms)))
        return theta, se, stats.reshape(-1)[:3 * nout].reshape(nout, 3), status[:nout], float(ms[0])

    def mvivw_robust(self, beta, weight, outcome, iv_off, iv, ex_off, ex, model=0, psi=2, want_rho=True):
        """`mvivw` by iteratively reweighted least squares (cusk_mvivw_robust; the rule is stated in include/cusk_hip.h):
        `psi` 1 Huber, 2 Huber then bisquare.  Returns (theta, se, stats, status, rho, kernel_ms): stats nout x 6 (rss,
        scale, tau, smallest squared pivot of the last weighted Gram, updates, sum of rho), rho in the layout of `iv`
        (None unless `want_rho`)."""
        beta, weight, outcome, iv_off, iv, ex_off, ex, theta, se, _, status = self._mvivw_args(
            beta, weight, outcome, iv_off, iv, ex_off, ex, None, None, None, None)
        (M, p), nout = beta.shape, outcome.shape[0]
        stats = np.full((max(nout, 1), 6), np.nan)
        rho = np.full(max(int(iv_off.max()), 1), np.nan) if want_rho else None
        ms = np.zeros(1, np.float32)
        self._check(lib().cusk_mvivw_robust(self.h, _ptr(beta), _ptr(weight), M, p, nout, _ptr(outcome), _ptr(iv_off), _ptr(iv),
                                            _ptr(ex_off), _ptr(ex), int(model), int(psi), _ptr(theta), _ptr(se), _ptr(stats),
                                            _ptr(status), _ptr(rho) if want_rho else None, _ptr(ms)))
        return theta, se, stats[:nout], status[:nout], rho, float(ms[0])

    def mvivw_jackknife(self, beta, weight, outcome, iv_off, iv, ex_off, ex, grp_off, grp, model=0, want_pres=True,
                        want_refit=True, guard=0):
        """`mvivw` with delete-group refits (cusk_mvivw_jackknife; the rule is stated in include/cusk_hip.h):
        `grp[grp_off[a]:grp_off[a + 1]]` are the group boundaries of outcome a, list positions strictly ascending from 0 to
        its number of instruments (`mvivw.groups` builds them).  Returns (theta, se, stats, status, jk, jk_arg, jk_stats,
        jk_status, pres, refit, kernel_ms): the first four as `mvivw`; jk nex x 4 (theta_J, se_J, min, max) and jk_arg at the
        positions of `ex`; jk_stats nout x 2 (PRESS, pivot); pres in the layout of `iv` and refit (theta_-g, outcome-major,
        then group, then exposure), each None unless wanted.  `guard`: that many extra entries behind every output array
        are filled with a mark and checked after the call (the tests' guard words)."""
        beta, weight, outcome, iv_off, iv, ex_off, ex, _, _, _, _ = self._mvivw_args(
            beta, weight, outcome, iv_off, iv, ex_off, ex, None, None, None, None)
        (M, p), nout = beta.shape, outcome.shape[0]
        grp_off = None if grp_off is None else np.ascontiguousarray(grp_off, np.int64).reshape(-1)
        grp = np.zeros(1, np.int32) if grp is None else np.ascontiguousarray(grp, np.int32).reshape(-1)
        if grp_off is not None:
            assert grp_off.shape[0] == nout + 1 and grp.shape[0] >= (int(grp_off.max()) if nout else 0)
            nrefit = int(np.sum(np.maximum(np.diff(grp_off) - 1, 0) * np.diff(ex_off))) if nout else 0
        else:
            nrefit = 0
        nex, niv = (int(ex_off.max()), int(iv_off.max())) if nout else (0, 0)
        MARK, IMARK = -777.0, -777
        sizes = dict(theta=nex, se=nex, stats=3 * nout, jk=4 * nex, jk_stats=2 * nout, pres=niv, refit=nrefit)
        out = {name: np.full(max(n, 1) + guard, MARK if guard else np.nan) for name, n in sizes.items()}
        ints = {name: np.full(max(n, 1) + guard, IMARK if guard else 0, np.int32)
                for name, n in dict(status=nout, jk_arg=nex, jk_status=nout).items()}
        ms = np.zeros(1, np.float32)
        self._check(lib().cusk_mvivw_jackknife(
            self.h, _ptr(beta), _ptr(weight), M, p, nout, _ptr(outcome), _ptr(iv_off), _ptr(iv), _ptr(ex_off), _ptr(ex),
            None if grp_off is None else _ptr(grp_off), _ptr(grp), int(model), _ptr(out["theta"]), _ptr(out["se"]),
            _ptr(out["stats"]), _ptr(ints["status"]), _ptr(out["jk"]), _ptr(ints["jk_arg"]), _ptr(out["jk_stats"]),
            _ptr(ints["jk_status"]), _ptr(out["pres"]) if want_pres else None, _ptr(out["refit"]) if want_refit else None,
            _ptr(ms)))
        if guard:
            sizes.update(status=nout, jk_arg=nex, jk_status=nout)
            for name, arr in {**out, **ints}.items():
                if not np.all(arr[max(sizes[name], 1):] == (IMARK if arr.dtype == np.int32 else MARK)):
                    raise RuntimeError(f"cusk_mvivw_jackknife wrote behind {name}")
        return (out["theta"][:max(nex, 1)], out["se"][:max(nex, 1)], out["stats"][:3 * nout].reshape(nout, 3), ints["status"][:nout],
                out["jk"][:4 * nex].reshape(nex, 4), ints["jk_arg"][:nex], out["jk_stats"][:2 * nout].reshape(nout, 2),
                ints["jk_status"][:nout], out["pres"][:max(niv, 1)] if want_pres else None,
                out["refit"][:max(nrefit, 1)] if want_refit else None, float(ms[0]))

    def abs_median(self, vals, seg_off, out=None):
        """The exact median of |vals[seg_off[g]:seg_off[g + 1]]| per segment (cusk_abs_median), NaN for an empty one.
        `out` may be given (float64, at least one entry per segment) to be filled in place."""
        vals = np.ascontiguousarray(vals, np.float64).reshape(-1)
        seg_off = np.ascontiguousarray(seg_off, np.int64).reshape(-1)
        nseg = seg_off.shape[0] - 1
        assert nseg >= 0 and vals.shape[0] >= (int(seg_off.max()) if nseg > 0 else 0)
        out = np.full(max(nseg, 1), np.nan) if out is None else out
        assert out.dtype == np.float64 and out.flags.c_contiguous and out.shape[0] >= nseg
        self._check(lib().cusk_abs_median(self.h, _ptr(vals), _ptr(seg_off), nseg, _ptr(out)))
        return out[:nseg]

    def corr_timing(self):
        t = np.zeros(4, np.float32)
        lib().cusk_corr_timing(self.h, _ptr(t))
        return t
