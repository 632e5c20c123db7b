"""Row-sharded engines in ONE process: `world` threads, one engine each, joined by a barrier and numpy.

`cusk_engine_set_row_shard` asks its caller for the collective (an element-wise unsigned MIN of one buffer per engine).
tools/row_shard_run.py supplies it with one process per rank and gloo; here the ranks are threads of the test process:
engines own private streams, `cusk_engine_bind_thread` makes the engine's device the thread's, and ctypes releases the
GIL while `cusk_run_*` runs.  The exchange of a rank copies its buffer into the group's slot (a pinned host copy is read
through a ctypes view, the device buffer through cusk_dev_download), waits on the barrier, takes the minimum over all
slots, waits again (nobody's slot is reused before everybody has read it), writes the result back and returns 0.  A
broken or timed-out barrier and any exception return 1: the engine must then fail, not wait.

Nothing here retries.  A thread that is still alive when the time limit of a run is over ends the pytest session
(`pytest.exit`): nothing further is started on a device on which a run hangs."""
import ctypes as C
import threading
import time
from dataclasses import dataclass, field

import numpy as np

BARRIER_TIMEOUT_S = 30
JOIN_TIMEOUT_S = 120


def _unsigned(elem_bytes):
    if elem_bytes not in (4, 8):
        raise ValueError(f"elem_bytes must be 4 or 8, not {elem_bytes}")
    return np.uint32 if elem_bytes == 4 else np.uint64


def unsigned_min(buffers, elem_bytes):
    """element-wise minimum of the participants' buffers (equal byte length, any integer dtype of `elem_bytes` bytes),
    every element compared as an unsigned integer -> a new array of uint32 / uint64.  "None" is all ones: the largest
    unsigned value, so it loses to everything else"""
    dt = _unsigned(elem_bytes)
    views = [np.ascontiguousarray(b).view(dt).reshape(-1) for b in buffers]
    if not views or any(v.shape != views[0].shape for v in views):
        raise ValueError("unsigned_min: one buffer per participant, all of one length")
    return np.minimum.reduce(views) if len(views) > 1 else views[0].copy()


def join_buffers(buffers, elem_bytes):
    """what the ranks of a group do together, in one call: every buffer (a writable contiguous array) ends up holding the
    unsigned minimum of all of them"""
    out = unsigned_min(buffers, elem_bytes)
    for b in buffers:
        b.view(_unsigned(elem_bytes)).reshape(-1)[:] = out
    return out


@dataclass
class RankResult:
    rank: int
    stats: object = None
    adjacency: np.ndarray = None
    sepsets: tuple = None  # (x, y, level, z, S) of Engine.sepsets(); None in hetcor mode
    pmax: np.ndarray = None  # None when make_run names no matrix
    calls: list = field(default_factory=list)  # (level, count, elem_bytes, on_device) of every exchange call of the run
    error: BaseException = None


class ShardGroup:
    """`world` engines on device 0 with `options`, row-sharded over each other (world = 1: one plain engine, no exchange).
    run() may be called repeatedly; close() destroys the engines."""

    def __init__(self, world, options=None, device_buffers=False):
        import cigwas_amd as cg

        self.world = int(world)
        self.device_buffers = bool(device_buffers)
        self.engines = []
        self.calls = [[] for _ in range(self.world)]
        self._wrap = None
        self._slots = [None] * self.world
        self._barrier = threading.Barrier(self.world, timeout=BARRIER_TIMEOUT_S)
        try:
            for r in range(self.world):
                e = cg.Engine(0)
                self.engines.append(e)
                for k, v in (options or {}).items():
                    e.set_option(k, v)
                if self.world > 1:
                    e.set_row_shard(r, self.world, self._exchange_of(r), host_staging=not self.device_buffers)
        except BaseException:
            self.close()
            raise

    def close(self):
        for e in self.engines:
            e.close()
        self.engines = []

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _join(self, rank, level, mine):
        """the working collective: unsigned MIN over every rank's copy"""
        elem = mine.itemsize
        self._slots[rank] = mine
        self._barrier.wait()
        out = unsigned_min(self._slots, elem)
        self._barrier.wait()  # (everybody has read every slot: they may be filled again)
        return out

    def _exchange_of(self, rank):
        from cigwas_amd._lib import lib

        def exchange(level, buf, count, elem_bytes, on_device, stream):
            self.calls[rank].append((int(level), int(count), int(elem_bytes), int(on_device)))
            try:
                dt = _unsigned(elem_bytes)
                if on_device:
                    mine = np.empty(count, dt)
                    if count and lib().cusk_dev_download(mine.ctypes.data_as(C.c_void_p), C.c_void_p(buf), mine.nbytes) != 0:
                        return 1
                    view = None
                else:
                    ctype = C.c_uint32 if elem_bytes == 4 else C.c_uint64
                    view = np.ctypeslib.as_array(C.cast(buf, C.POINTER(ctype)), shape=(count,)) if count else np.empty(0, dt)
                    mine = view.copy()
                join = self._wrap(self._join) if self._wrap else self._join
                out = join(rank, level, mine)
                if out is None:
                    return 1
                out = np.ascontiguousarray(out, dt)
                if out.shape != (count,):
                    return 1
                if view is not None:
                    view[:] = out
                elif count and lib().cusk_dev_upload(C.c_void_p(buf), out.ctypes.data_as(C.c_void_p), out.nbytes) != 0:
                    return 1
                return 0
            except Exception:  # threading.BrokenBarrierError (a rank missing or late) included
                return 1

        return exchange

    def run(self, make_run, exchange_wrap=None, return_errors=False):
        """One thread per engine: cusk_engine_bind_thread, then make_run(engine) -> stats or (stats, C_dev); the thread
        then reads the engine's adjacency, its separating sets (Skeleton runs) and, given C_dev, pMax.
        exchange_wrap(join) -> join', with join(rank, level, mine) -> the array to write back (None: the exchange fails),
        substitutes the collective on every rank.  -> [RankResult]; an exception of a rank is raised here unless
        return_errors, which leaves it in RankResult.error"""
        import pytest
        from cigwas_amd._lib import lib

        self._wrap = exchange_wrap
        self._barrier.reset()
        for c in self.calls:
            c.clear()
        results = [RankResult(r) for r in range(self.world)]

        def work(r):
            res, e = results[r], self.engines[r]
            try:
                if lib().cusk_engine_bind_thread(e.h) != 0:
                    raise RuntimeError("cusk_engine_bind_thread failed")
                got = make_run(e)
                res.stats, C_dev = got if isinstance(got, tuple) else (got, None)
                res.adjacency = e.adjacency()
                if lib().cusk_result_sepsets(e.h, None, None, None, None, None) >= 0:
                    res.sepsets = e.sepsets()
                if C_dev is not None:
                    res.pmax = e.pmax(C_dev)
            except BaseException as exc:  # noqa: BLE001 -- handed to the caller
                res.error = exc

        threads = [threading.Thread(target=work, args=(r,), daemon=True, name=f"shard-rank-{r}") for r in range(self.world)]
        for t in threads:
            t.start()
        deadline = time.monotonic() + JOIN_TIMEOUT_S
        for t in threads:
            t.join(max(0.0, deadline - time.monotonic()))
        stuck = [r for r, t in enumerate(threads) if t.is_alive()]
        if stuck:
            where = ", ".join(f"rank {r} (last exchange at level {self.calls[r][-1][0] if self.calls[r] else 'none'})" for r in stuck)
            pytest.exit(f"row-sharded run of {self.world} engines still running after {JOIN_TIMEOUT_S} s: {where}; "
                        "nothing more is started on the device", returncode=1)
        for r, res in enumerate(results):
            res.calls = list(self.calls[r])
        if not return_errors:
            for res in results:
                if res.error is not None:
                    raise res.error
        return results


def run_sharded(world, make_run, options=None, device_buffers=False, exchange_wrap=None, return_errors=False):
    """ShardGroup(world, options, device_buffers).run(make_run, exchange_wrap) on engines of its own -> [RankResult]"""
    with ShardGroup(world, options, device_buffers) as g:
        return g.run(make_run, exchange_wrap, return_errors)
