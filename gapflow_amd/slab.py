"""x-slab decomposition of one problem over the GPUs of a node: one process per GPU.

The reference is single-process (README.md:60-61); this module is new.  The grid is cut along x
(the slow axis of the device planes, so halo rows are contiguous).  A fused step needs its
neighbours' field only one row deep (the composed MacCormack stencil has radius 1, see
csrc/step_kernel.hip), so per time step each rank needs ONE row from each neighbour plus everybody's 64-byte record
(sum Ekin, max v^2, max c^2, validity).  Both travel in a single all-gather after the stencil
kernel, before the dt/residual commit:

    gpf_step_local   (stage-1 ghost data + fused stencil + local ghost rules + message: first row, last row, record)
    all_gather_into_tensor(gathered, message)               <- torch.distributed (RCCL over xGMI)
    gpf_step_commit  (scatter the neighbours' rows, reduce records in rank order, advance dt/residual)

Everything is enqueued on one stream; there is no host synchronisation inside `advance`.
With domain series armed (SlabProblem.set_domain_series: the film integrals and the field extrema of the whole domain, on every
rank) a step that takes the count to a due multiple is followed, on the same stream, by

    gpf_slab_series_local   (this rank's rows reduced to one vector each, into the series message)
    all_gather_into_tensor(series gathered, series message)
    gpf_slab_series_fold    (all rows folded in the undivided order: every rank holds the undivided problem's record)

Reductions are combined in rank order on every rank, so all ranks hold bit-identical dt.

Kinds of a slab's outer rows (gpf_config.halo_lo/hi): 0 physical ghost row (local rule),
1 copy of the neighbour's interior row, 2 the domain's periodic ghost row (filled by the ring).

`SlabDriver` is backend-neutral (any engine with message / step_local / commit); the product
engine is `HipSlabEngine`.  tests/test_slab_gloo.py drives the same driver with a CPU engine over
gloo to check partitioning, message pairing and the rank-ordered reduction.
"""
import ctypes as C
import io as _io
import os
import sys
from copy import deepcopy

import numpy as np

from . import _lib
from .io import read_yaml_input
from .series import _Series, _domain_chunk, _domain_series_entry, _integral_sections
from .topography import Topography, topography_rows

HALO_PHYSICAL, HALO_NEIGHBOUR, HALO_SEAM = 0, 1, 2


def partition(Nx, world):
    """Global interior rows [lo, hi] (1-based, inclusive) of every rank; remainders go to the first ranks."""
    base, rem = divmod(Nx, world)
    if base < 1:
        raise ValueError(f"cannot cut Nx={Nx} rows into {world} slabs")
    out, lo = [], 1
    for r in range(world):
        n = base + (1 if r < rem else 0)
        out.append((lo, lo + n - 1))
        lo += n
    return out


class SlabLayout:
    """Everything a rank needs to know about its slab."""

    def __init__(self, grid, rank, world):
        self.rank, self.world = rank, world
        self.Nx_global = grid['Nx']
        self.lo, self.hi = partition(grid['Nx'], world)[rank]
        self.nx = self.hi - self.lo + 1
        periodic = all(grid['bc_xE_P']) and all(grid['bc_xW_P'])
        self.periodic = periodic
        first, last = rank == 0, rank == world - 1
        if world == 1:
            self.kind_lo = self.kind_hi = HALO_PHYSICAL
            self.lower = self.upper = None
        else:
            self.kind_lo = (HALO_SEAM if periodic else HALO_PHYSICAL) if first else HALO_NEIGHBOUR
            self.kind_hi = (HALO_SEAM if periodic else HALO_PHYSICAL) if last else HALO_NEIGHBOUR
            self.lower = (world - 1 if periodic else None) if first else rank - 1
            self.upper = (0 if periodic else None) if last else rank + 1

    def rows(self):
        """Slice of the global (Nx+2)-row arrays held by this rank, including its two outer rows."""
        return slice(self.lo - 1, self.hi + 2)

    def local_grid(self, grid):
        g = deepcopy(grid)
        g['Nx'] = self.nx
        g['Lx'] = grid['dx'] * self.nx
        return g


class LoopbackGroup:
    """One process standing in for rank `rank` of `world` (rehearsal and timing on a one-GPU box): every peer's contribution
    to a collective is this rank's own.  For a domain that repeats with the slab's period that is exactly what the real
    neighbours would send (tests/test_gpu_gp_large.py); for any other domain it exercises the rank's kernels, message
    sizes and launch sequence, not the physics across the slab boundary."""

    class ReduceOp:
        SUM, MAX, MIN = 'sum', 'max', 'min'

    def __init__(self, rank, world):
        self._rank, self._world = rank, world

    def get_rank(self):
        return self._rank

    def get_world_size(self):
        return self._world

    def all_gather_into_tensor(self, out, inp):
        out.view(self._world, -1).copy_(inp.view(1, -1).expand(self._world, -1))

    def all_reduce(self, t, op=None):
        if op == self.ReduceOp.SUM:
            t.mul_(self._world)

    def broadcast_object_list(self, box, src=0):
        pass

    def all_to_all_single(self, out, inp, output_split_sizes, input_split_sizes):
        """Chunk s of the output is the start of this rank's own chunk for s (message sizes and launches, not physics)."""
        oo, io = 0, 0
        for n_out, n_in in zip(output_split_sizes, input_split_sizes):
            n = min(n_out, n_in)
            out[oo:oo + n].copy_(inp[io:io + n])
            out[oo + n:oo + n_out].zero_()
            oo, io = oo + n_out, io + n_in

    def barrier(self):
        pass


class HostStagedGroup:
    """torch.distributed look-alike that moves GPU tensors through host memory over a CPU backend (gloo).

    RCCL refuses two ranks on one device ("Duplicate GPU detected"), so on a one-GPU box the multi-rank behaviour of the
    HIP slab engine (halo kinds, seam topography, message rows, rank-ordered commit) is rehearsed with a few processes
    sharing the GPU and this transport (tests/test_gpu_slab.py, bench.py with GPF_BENCH_ONE_GPU_REHEARSAL=1)."""

    def __init__(self, dist, torch):
        self._d, self._t = dist, torch
        self.ReduceOp = dist.ReduceOp

    def get_rank(self):
        return self._d.get_rank()

    def get_world_size(self):
        return self._d.get_world_size()

    def all_gather_into_tensor(self, out, inp):
        self._t.cuda.synchronize()
        o, i = out.cpu(), inp.cpu()
        self._d.all_gather_into_tensor(o, i)
        out.copy_(o)

    def all_reduce(self, t, op=None):
        c = t.cpu()
        self._d.all_reduce(c, op=op if op is not None else self.ReduceOp.SUM)
        t.copy_(c)

    def all_to_all_single(self, out, inp, output_split_sizes, input_split_sizes):
        self._t.cuda.synchronize()
        o, i = out.cpu(), inp.cpu()
        self._d.all_to_all_single(o, i, output_split_sizes, input_split_sizes)      # gloo: alltoall_base
        out.copy_(o)

    def broadcast_object_list(self, box, src=0):
        self._d.broadcast_object_list(box, src=src)

    def barrier(self):
        self._d.barrier()

    def destroy_process_group(self):
        self._d.destroy_process_group()


class ThreadWorld:
    """N ranks as N THREADS of one process, all on one GPU: `run(fn)` calls fn(group) once per rank, each with its own
    torch.distributed look-alike whose collectives meet at thread barriers and move data with device copies.

    What it is for: the test boxes allow six processes on a card, so an 8-rank decomposition (BASELINE.json configs[4], the
    8-slab strong-scaling run) cannot be rehearsed with one process per rank there.  Every rank is a real SlabProblem with
    its own library handle, partition, halo kinds, seam topography and messages; only the transport is stood in for.  All
    ranks enqueue on the device's default stream, so "every rank has enqueued its part" (a thread barrier) is all the
    ordering a collective needs.  All-gather and all-to-all transport only: the mailbox kernels poll for their peers and would
    wait for launches queued behind them on the shared stream."""

    class ReduceOp:
        SUM, MAX, MIN = 'sum', 'max', 'min'

    def __init__(self, world, torch):
        import threading
        self.world, self.torch = world, torch
        self._barrier = threading.Barrier(world)
        self._slots = [None] * world

    class _Group:
        def __init__(self, w, rank):
            self._w, self._rank = w, rank
            self.ReduceOp = ThreadWorld.ReduceOp

        def get_rank(self):
            return self._rank

        def get_world_size(self):
            return self._w.world

        def barrier(self):
            self._w._barrier.wait()

        def all_gather_into_tensor(self, out, inp):
            w = self._w
            w._slots[self._rank] = inp
            w._barrier.wait()                           # every rank's producers are enqueued
            parts = out.view(w.world, -1)
            for r in range(w.world):
                parts[r].copy_(w._slots[r].view(-1))
            w._barrier.wait()                           # every rank's copies are enqueued: the inputs may change again

        def all_to_all_single(self, out, inp, output_split_sizes, input_split_sizes):
            """Uneven all-to-all: chunk r of rank s's input goes to chunk s of rank r's output (device copies)."""
            w = self._w
            w._slots[self._rank] = (inp, list(input_split_sizes))
            w._barrier.wait()                           # every rank's producers are enqueued
            o = 0
            for s in range(w.world):
                src, splits = w._slots[s]
                n, start = output_split_sizes[s], sum(splits[:self._rank])
                if splits[self._rank] != n:
                    raise ValueError(f"all_to_all_single: rank {s} sends {splits[self._rank]} elements, rank {self._rank} expects {n}")
                if n:
                    out[o:o + n].copy_(src[start:start + n])
                o += n
            w._barrier.wait()                           # every rank's copies are enqueued: the inputs may change again

        def all_reduce(self, t, op=None):
            w, torch = self._w, self._w.torch
            w._slots[self._rank] = t.clone()
            w._barrier.wait()
            stack = torch.stack([w._slots[r] for r in range(w.world)])      # rank order on every rank
            res = stack.sum(0) if op in (None, 'sum') else (stack.max(0).values if op == 'max' else stack.min(0).values)
            w._barrier.wait()
            t.copy_(res)

        def broadcast_object_list(self, box, src=0):
            w = self._w
            if self._rank == src:
                w._slots[src] = list(box)
            w._barrier.wait()
            box[:] = w._slots[src]
            w._barrier.wait()

    def run(self, fn):
        """fn(group) on every rank; returns the results in rank order.  The first exception breaks the barriers (the other
        ranks then fail at their next collective) and is re-raised."""
        import threading
        results, errors = [None] * self.world, []

        def body(rank):
            try:
                if self.torch.cuda.is_available():
                    self.torch.cuda.set_device(0)
                results[rank] = fn(ThreadWorld._Group(self, rank))
            except threading.BrokenBarrierError:
                pass
            except BaseException as e:      # noqa: BLE001
                errors.append((rank, e))
                self._barrier.abort()

        threads = [threading.Thread(target=body, args=(r,), name=f'slab-rank-{r}') for r in range(self.world)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        if errors:
            rank, e = sorted(errors, key=lambda x: x[0])[0]
            raise RuntimeError(f"rank {rank} of the thread world failed: {type(e).__name__}: {e}") from e
        return results


class SlabDriver:
    """Runs the split step of an engine: step_local -> ONE all-gather -> commit.

    Every rank contributes one message [first row | last row | record]; after the all-gather each rank picks its
    neighbours' rows out of the gathered buffer.  (Point-to-point sends would move 8x fewer bytes, but the rows are
    ~100 KB and a step is latency-bound: one collective instead of an all-gather plus a send/recv group halves both
    the host dispatch and the number of RCCL kernels per step.)"""

    def __init__(self, engine, layout, dist, torch):
        self.engine, self.layout, self.dist = engine, layout, dist
        self.message = engine.message()
        self.gathered = torch.zeros(self.message.numel() * layout.world, dtype=torch.float64, device=self.message.device)
        # rank whose LAST row is my row 0 / whose FIRST row is my row Nx+1
        self.rank_lo = -1 if layout.lower is None else layout.lower
        self.rank_hi = -1 if layout.upper is None else layout.upper

        self.torch = torch
        self.enqueued = 0               # steps issued since pre_run (the predictor direction may alternate with it)
        self.graph = None
        self.graph_honor = None
        self.use_graph = os.environ.get('GPF_SLAB_GRAPH', '0') == '1' and self.message.is_cuda
        self.p2p = False                # True: the step's own kernels exchange rows and records (gpf_step_p2p)
        self.series = None              # armed domain series (SlabProblem.set_domain_series): begin / chunk / due / local / fold / end

    def _eager(self, n, honor_stop):
        for _ in range(n):
            self.engine.step_local(honor_stop)
            self.dist.all_gather_into_tensor(self.gathered, self.message)
            self.engine.commit(self.gathered, honor_stop, self.rank_lo, self.rank_hi)
        self.enqueued += n

    def _recording(self, n, honor_stop):
        """n eager steps with the domain series armed: behind the commit of a step that takes the count to a due multiple, the
        partials of the series due, ONE all-gather of the series message and the folds, all on the stream of the step and
        without host synchronisation in between.  The series' begin / end bracket each piece (they read the state, before the
        first launch and after the last); a call that would leave more records than the device buffers hold is taken in pieces,
        and a run that stopped on the device ends the call."""
        s, done = self.series, 0
        while done < n:
            base = s.begin()
            piece = s.chunk(base, n - done)
            for i in range(piece):
                self.engine.step_local(honor_stop)
                self.dist.all_gather_into_tensor(self.gathered, self.message)
                self.engine.commit(self.gathered, honor_stop, self.rank_lo, self.rank_hi)
                if s.due(base + i + 1):
                    s.local(base + i + 1)
                    self.dist.all_gather_into_tensor(s.gathered, s.message)
                    s.fold(base + i + 1)
            self.enqueued += piece
            done += piece
            if s.end() < piece:
                break

    def _capture(self, honor_stop):
        """Record two consecutive steps (an even and an odd one: MC_order 0 alternates the sweep direction,
        problem.py:521-522) -- library kernels and the RCCL all-gather -- into one hipGraph."""
        torch = self.torch
        g = torch.cuda.CUDAGraph()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            self.engine.set_stream(side.cuda_stream)
            try:
                with torch.cuda.graph(g, stream=side):
                    for _ in range(2):
                        self.engine.step_local(honor_stop)
                        self.dist.all_gather_into_tensor(self.gathered, self.message)
                        self.engine.commit(self.gathered, honor_stop, self.rank_lo, self.rank_hi)
            finally:
                self.engine.set_stream(torch.cuda.current_stream().cuda_stream)
        torch.cuda.current_stream().wait_stream(side)
        self.engine.set_stream(torch.cuda.current_stream().cuda_stream)
        self.graph, self.graph_honor = g, honor_stop

    def advance(self, n, honor_stop=False):
        """n time steps; with GPF_SLAB_GRAPH=1 pairs of steps are replayed from a captured hipGraph, which takes
        the per-step host dispatch (two library calls and one collective) off the critical path."""
        if self.series is not None:             # eager, whatever GPF_SLAB_GRAPH says: a captured pair of steps has no room for a record
            if self.p2p:
                raise NotImplementedError("domain series: not recorded over the peer-to-peer transport (its batches have no host between steps)")
            return self._recording(n, honor_stop)
        if self.p2p:
            self.engine.step_p2p(n, honor_stop)
            self.enqueued += n
            return
        if not self.use_graph or n < 6:
            return self._eager(n, honor_stop)
        if self.enqueued == 0:
            self._eager(2, honor_stop)          # first calls allocate and plan: keep them out of the capture
            n -= 2
        if self.enqueued % 2:
            self._eager(1, honor_stop)
            n -= 1
        if self.graph is None or self.graph_honor != honor_stop:
            self._capture(honor_stop)           # capturing does not execute
        for _ in range(n // 2):
            self.graph.replay()
        self.enqueued += 2 * (n // 2)
        self.engine.resync()                    # the library's own step counter did not see the replays
        self._eager(n % 2, honor_stop)


class _DeviceArray:
    """Exposes library-owned device memory to torch through the CUDA array interface (no copy)."""

    def __init__(self, ptr, n):
        self.__cuda_array_interface__ = {'shape': (n,), 'typestr': '<f8', 'data': (int(ptr), False), 'version': 2}


class HipSlabEngine:
    """The product engine: one libgapflow_hip handle per rank."""

    def __init__(self, lib, handle, torch, world):
        self.lib, self.h, self.torch, self.world = lib, handle, torch, world
        p, n = C.c_void_p(), C.c_size_t(0)
        _lib.check(lib.gpf_slab_message(handle, C.byref(p), C.byref(n)))
        self._msg = torch.as_tensor(_DeviceArray(p.value, n.value), device='cuda')

    def message(self):
        return self._msg

    def step_local(self, honor_stop):
        _lib.check(self.lib.gpf_step_local(self.h, int(honor_stop)))

    def commit(self, gathered, honor_stop, rank_lo, rank_hi):
        _lib.check(self.lib.gpf_step_commit(self.h, int(honor_stop), C.c_void_p(gathered.data_ptr()), self.world,
                                            int(rank_lo), int(rank_hi)))

    def step_p2p(self, n, honor_stop):
        _lib.check(self.lib.gpf_step_p2p(self.h, int(n), int(honor_stop)))

    def set_stream(self, stream_ptr):
        _lib.check(self.lib.gpf_set_stream(self.h, C.c_void_p(stream_ptr)))

    def resync(self):
        sc = _lib.GpfScalars()
        _lib.check(self.lib.gpf_state(self.h, C.byref(sc)))     # synchronises; re-reads the device step counter


class _DomainFeatures:
    """The whole domain's (ncell, 7) feature table [rho, jx, jy, h, dh/dx, dh/dy, extra] of the initial state, rows on
    demand: what Database.initialize asks of its `Xtest` (column means of the uniform initial field, the number of
    cells, the features of a few hundred sampled cells) without a 3.8 GB table per rank at 8192^2."""

    def __init__(self, q0, grid, topo_rows):
        self._q0, self._topo_rows = np.asarray(q0, float), topo_rows
        self._ny2 = grid['Ny'] + 2
        self.shape = ((grid['Nx'] + 2) * self._ny2, 7)

    def column_mean(self, k):
        if k > 2:
            raise NotImplementedError("only the (uniform) initial field has a mean here")
        return float(self._q0[k])

    def rows(self, cells):
        cells = np.asarray(cells, int)
        ix, iy = cells // self._ny2, cells % self._ny2
        uniq, inv = np.unique(ix, return_inverse=True)
        t = self._topo_rows(uniq)                           # (3, len(uniq), Ny+2)
        out = np.zeros((len(cells), 7))
        out[:, :3] = self._q0
        out[:, 3:6] = t[:, inv, iy].T
        return out


class _CommittedSteps:
    """What _Series.collect asks of a stepping call's scalar records -- how many steps it committed and the simulated time of the
    recorded ones -- for a slab, which keeps no per-step log on the host: the times come with the records (gpf_slab_series_read),
    and the read fills them in here."""

    class _Entry:
        def __init__(self, simtime):
            self.simtime = simtime

    def __init__(self, before, ran):
        self.before, self.ran, self.times = before, ran, {}

    def __len__(self):
        return self.ran

    def __getitem__(self, k):
        return self._Entry(self.times[self.before + k + 1])


class _DomainSeries:
    """One rank's half of the armed domain series (SlabProblem.set_domain_series): the library's recorder (gpf_slab_series_*), its
    message and the gathered messages as torch tensors, and the host's records -- one series._Series per armed series.  The
    driver calls begin / chunk / due / local / fold / end (SlabDriver._recording); `now` is the record of the current state."""

    def __init__(self, slab, integrals, extrema, sx, sy):
        self.lib, self.h, L, t = slab.lib, slab._h, slab.layout, slab.torch
        self.strides, self.sections = (integrals, extrema), (sx, sy)
        i32p = C.POINTER(C.c_int32)
        ax, ay = np.array(sx, dtype=np.int32), np.array(sy, dtype=np.int32)
        _lib.check(self.lib.gpf_slab_series_set(self.h, L.lo - 1, L.Nx_global, L.world, integrals, len(sx), ax.ctypes.data_as(i32p),
                                                len(sy), ay.ctypes.data_as(i32p), extrema))
        p, n = C.c_void_p(), C.c_size_t(0)
        _lib.check(self.lib.gpf_slab_series_message(self.h, C.byref(p), C.byref(n)))
        self.message = t.as_tensor(_DeviceArray(p.value, n.value), device='cuda')
        self.gathered = t.zeros(n.value * L.world, dtype=t.float64, device='cuda')
        self.nrec = len(_lib.INTEGRAL_SUMS) + len(sx) + len(sy)
        self.reset()

    def reset(self):
        """The series start afresh (set_domain_series, pre_run)."""
        integrals, extrema = self.strides
        self.film = _Series('domain integrals', integrals) if integrals else None
        self.ext = _Series('domain extrema', extrema) if extrema else None
        self._base = 0

    def clear(self):
        _lib.check(self.lib.gpf_slab_series_clear(self.h))

    def begin(self):
        base = C.c_int64(0)
        _lib.check(self.lib.gpf_slab_series_begin(self.h, C.byref(base)))
        self._base = int(base.value)
        return self._base

    def chunk(self, base, n):
        return _domain_chunk(base, n, self.strides, _lib.LOG_CAPACITY)

    def due(self, expect):
        return any(every and expect % every == 0 for every in self.strides)

    def local(self, expect):
        _lib.check(self.lib.gpf_slab_series_local(self.h, expect))

    def fold(self, expect):
        _lib.check(self.lib.gpf_slab_series_fold(self.h, C.c_void_p(self.gathered.data_ptr()), self.gathered.numel(), expect))

    def end(self):
        """The records of the steps the call committed -> the host's series; how many steps that were."""
        ran = C.c_int64(0)
        _lib.check(self.lib.gpf_slab_series_end(self.h, C.byref(ran)))
        nq, i32p = len(_lib.EXTREMA_NAMES), C.POINTER(C.c_int32)
        for which, rec, shapes in ((0, self.film, [((self.nrec,), np.float64)]), (1, self.ext, [((nq,), np.float64), ((nq, 2), np.int32)])):
            if rec is None or ran.value < 1:
                continue
            entries = _CommittedSteps(self._base, int(ran.value))

            def read(b, n, steps, have, which=which, entries=entries):
                times = np.zeros(n)
                cells = b[1].ctypes.data_as(i32p) if which == 1 else None
                _lib.check(self.lib.gpf_slab_series_read(self.h, which, _lib.as_dp(b[0]), cells, _lib.as_dp(times), n, steps, have))
                entries.times = {int(steps[k]): times[k] for k in range(n)}
            rec.collect(read, entries, self._base, shapes)
        return int(ran.value)

    def now(self, dist):
        """Both records of the current state, as the library hands them out: (integrals [nrec], values [7], cells [7][2]).  Collective."""
        _lib.check(self.lib.gpf_slab_series_now_local(self.h))
        dist.all_gather_into_tensor(self.gathered, self.message)
        nq = len(_lib.EXTREMA_NAMES)
        out, vals, cells = np.empty(self.nrec), np.empty(nq), np.zeros((nq, 2), dtype=np.int32)
        _lib.check(self.lib.gpf_slab_series_now_fold(self.h, C.c_void_p(self.gathered.data_ptr()), self.gathered.numel(), _lib.as_dp(out), out.size,
                                                     _lib.as_dp(vals), cells.ctypes.data_as(C.POINTER(C.c_int32))))
        return out, vals, cells


class SlabProblem:
    """A Problem cut into x-slabs; construct it on every rank of an initialised process group."""

    def gap_profiles(self, *args, **kwargs):
        """Through-gap profiles are not evaluated on x-slabs: gather the state and use Problem.gap_profiles or
        gapflow_amd.models.profiles on it."""
        raise NotImplementedError("gap_profiles: not available on a SlabProblem")

    def set_probes(self, *args, **kwargs):
        """Point probes are recorded on unsliced problems only."""
        raise NotImplementedError("probes: not available on a SlabProblem")

    def set_integrals(self, *args, **kwargs):
        """Film integrals are reduced on unsliced problems only."""
        raise NotImplementedError("integrals: not available on a SlabProblem (the whole domain's: set_domain_series / domain_film_integrals)")

    def film_integrals(self, *args, **kwargs):
        """Film integrals are reduced on unsliced problems only."""
        raise NotImplementedError("integrals: not available on a SlabProblem (the whole domain's: set_domain_series / domain_film_integrals)")

    def set_weighted_integrals(self, *args, **kwargs):
        """Weighted film integrals are reduced on unsliced problems only."""
        raise NotImplementedError("weighted integrals: not available on a SlabProblem")

    def film_weighted(self, *args, **kwargs):
        """Weighted film integrals are reduced on unsliced problems only."""
        raise NotImplementedError("weighted integrals: not available on a SlabProblem")

    def set_regions(self, *args, **kwargs):
        """Regions are reduced on unsliced problems only."""
        raise NotImplementedError("regions: not available on a SlabProblem")

    def film_regions(self, *args, **kwargs):
        """Regions are reduced on unsliced problems only."""
        raise NotImplementedError("regions: not available on a SlabProblem")

    def set_lines(self, *args, **kwargs):
        """Line profiles are recorded on unsliced problems only."""
        raise NotImplementedError("lines: not available on a SlabProblem")

    def film_lines(self, *args, **kwargs):
        """Line profiles are recorded on unsliced problems only."""
        raise NotImplementedError("lines: not available on a SlabProblem")

    def set_frames(self, *args, **kwargs):
        """Reduced frames are recorded on unsliced problems only (`options.frames` is stored and never armed here)."""
        raise NotImplementedError("frames: not available on a SlabProblem")

    def frame_now(self, *args, **kwargs):
        """Reduced frames are taken on unsliced problems only."""
        raise NotImplementedError("frames: not available on a SlabProblem")

    def set_extrema(self, *args, **kwargs):
        """Field extrema are recorded on unsliced problems only."""
        raise NotImplementedError("extrema: not available on a SlabProblem (the whole domain's: set_domain_series / domain_field_extrema)")

    def field_extrema(self, *args, **kwargs):
        """Field extrema are taken on unsliced problems only."""
        raise NotImplementedError("extrema: not available on a SlabProblem (the whole domain's: set_domain_series / domain_field_extrema)")

    def set_elastic_series(self, *args, **kwargs):
        """The deformation series is recorded on unsliced problems only."""
        raise NotImplementedError("elastic series: not available on a SlabProblem")

    def film_elastic(self, *args, **kwargs):
        """The deformation series is taken on unsliced problems only."""
        raise NotImplementedError("elastic series: not available on a SlabProblem")

    def set_thinning_series(self, *args, **kwargs):
        """The thinning series is recorded on unsliced problems only (options.thinning_series is kept and never armed here)."""
        raise NotImplementedError("thinning series: not available on a SlabProblem")

    def film_thinning(self, *args, **kwargs):
        """The thinning series is taken on unsliced problems only."""
        raise NotImplementedError("thinning series: not available on a SlabProblem")

    def set_changes(self, *args, **kwargs):
        """Step changes are recorded on unsliced problems only."""
        raise NotImplementedError("changes: not available on a SlabProblem")

    def step_change(self, *args, **kwargs):
        """Step changes are taken on unsliced problems only."""
        raise NotImplementedError("changes: not available on a SlabProblem")

    def set_statistics(self, *args, **kwargs):
        """Running field statistics are kept on unsliced problems only."""
        raise NotImplementedError("statistics: not available on a SlabProblem")

    @property
    def statistics(self):
        """Running field statistics are kept on unsliced problems only."""
        raise NotImplementedError("statistics: not available on a SlabProblem")

    def init_from(self, *args, **kwargs):
        """States are resampled onto unsliced problems only."""
        raise NotImplementedError("init_from: not available on a SlabProblem")

    def __init__(self, input_dict, device=0, dist=None):
        opts = input_dict.get('options') or {}
        # the options that arm what the methods above refuse are refused as those are
        for key, label in (('init_from', 'init_from'), ('probes', 'probes'), ('integrals', 'integrals'),
                           ('weighted_integrals', 'weighted integrals'), ('regions', 'regions'), ('lines', 'lines'), ('extrema', 'extrema'),
                           ('elastic_series', 'elastic series'), ('statistics', 'statistics'), ('changes', 'changes')):
            given = opts.get(key)
            if given is not None if key in ('probes', 'integrals') else given:      # (the others: 0 is off, as on a Problem)
                raise NotImplementedError(f"{label}: not available on a SlabProblem" +
                                          (" (the whole domain's: options.domain_series)" if key in ('integrals', 'extrema') else ""))
        import torch
        if dist is None:
            import torch.distributed as dist
        self.torch, self.dist = torch, dist
        self._device, self._writer_problem, self._pre_run_done = device, None, False
        self._restart_history = None            # rank 0 after load_checkpoint: the saved run's frame history
        self.rank, self.world = dist.get_rank(), dist.get_world_size()
        self.input = input_dict
        grid, prop, geo = input_dict['grid'], input_dict['properties'], input_dict['geometry']
        self.layout = L = SlabLayout(grid, self.rank, self.world)
        self.lib = _lib.require_device()

        # the serial problem's configuration, narrowed to this slab
        from .problem import Problem
        shell = Problem.__new__(Problem)
        shell.options, shell.numerics, shell.prop, shell.geo = input_dict['options'], input_dict['numerics'], prop, geo
        shell.grid = L.local_grid(grid)
        cfg = shell._make_config(device)
        # shear thinning: the viscosity of a halo row depends on grad p there, i.e. on a second row of the neighbour -- the
        # stage-wise step then exchanges two rows per side (gpf_upload_beyond / gpf_stage_message) and is the only step
        self._thinning = bool(cfg.thinning)
        if self._thinning and L.nx < 2 and self.world > 1:
            raise ValueError("shear thinning across slabs needs at least two rows per slab")
        cfg.halo_lo, cfg.halo_hi = L.kind_lo, L.kind_hi
        self.grid_local = shell.grid
        self._h = C.c_void_p()
        _lib.check(self.lib.gpf_create(C.byref(cfg), C.byref(self._h)))
        _lib.check(self.lib.gpf_set_stream(self._h, C.c_void_p(torch.cuda.current_stream().cuda_stream)))

        # this slab's rows of the domain's topography (never the whole table: 2 GB per rank at 8192^2)
        hmins = self._shared_asperity_heights(geo)
        if geo.get('flip'):
            whole = Topography(grid, geo, prop).full[:3]
            topo_rows = lambda rows: whole[:, np.asarray(rows)]
        else:
            topo_rows = lambda rows: topography_rows(grid, geo, rows, hmins)
        self._topo_rows = topo_rows
        shape = (L.nx + 2, grid['Ny'] + 2)
        self._shape = shape
        topo_local = topo_rows(np.arange(L.lo - 1, L.hi + 2))
        self._upload(_lib.FIELD_TOPO, topo_local)
        q = np.empty((3,) + shape)
        q[0], q[1], q[2] = prop['rho0'], prop['rho0'] * geo['U'] / 2.0, prop['rho0'] * geo['V'] / 2.0
        self._upload(_lib.FIELD_Q, q)
        if self._thinning:
            beyond = _lib.f64c(np.full(grid['Ny'] + 2, prop['rho0']))          # the uniform initial field, one row further
            for side, kind in ((0, L.kind_lo), (1, L.kind_hi)):
                if kind == HALO_NEIGHBOUR:
                    _lib.check(self.lib.gpf_upload_beyond(self._h, side, _lib.as_dp(beyond), beyond.size))
        nxg = grid['Nx']
        for side, kind, (r_src, r_up) in ((0, L.kind_lo, (nxg, nxg + 1)), (1, L.kind_hi, (1, 0))):
            if kind == HALO_SEAM:
                seam = np.zeros((2, 4, grid['Ny'] + 2))
                two = topo_rows([r_src, r_up])
                seam[0, :3], seam[1, :3] = two[:, 0], two[:, 1]
                seam = _lib.f64c(seam)
                _lib.check(self.lib.gpf_set_seam_topo(self._h, side, _lib.as_dp(seam), seam.size))
        self.engine = HipSlabEngine(self.lib, self._h, torch, self.world)
        self.driver = SlabDriver(self.engine, L, dist, torch)
        self._elastic, self._domain = None, None
        if prop.get('elastic', {}).get('enabled', False):
            self._elastic = SlabElastic(self, grid, prop['elastic'], topo_rows)

        # surrogate closures: the database and the models are replicated on every rank
        self.grid, self._lib, self._closures_stale = grid, self.lib, True
        self._topo_local = topo_local
        self._extra = np.zeros((1,) + shape)
        self._features_global = _DomainFeatures(q[:, 0, 0], grid, topo_rows)
        self.database, self._gp_models = None, {}
        gp = input_dict.get('gp')
        if input_dict.get('db') is not None:
            from .gp import make_database
            self.database = make_database(input_dict, device)
        if gp is not None:
            if self.database is None:
                raise IOError("a `gp` section needs a `db` section")
            from .gp import attach_surrogates, SlabSurrogate
            self._gp_models = attach_surrogates(self, gp, self.database, cls=SlabSurrogate)
            self._pair = torch.zeros(8, dtype=torch.float64, device='cuda')
            self._pairs = torch.zeros(8 * self.world, dtype=torch.float64, device='cuda')

        if os.environ.get('GPF_SLAB_TRANSPORT', 'rccl') == 'p2p':
            if not self.connect_p2p():
                raise RuntimeError("GPF_SLAB_TRANSPORT=p2p: the peers' mailboxes could not be mapped (HIP IPC)")
        ds = opts.get('domain_series')              # options.domain_series (from the YAML text, or carried by a checkpoint's dictionaries)
        if ds and (ds.get('integrals') or ds.get('extrema')):
            self.set_domain_series(ds.get('integrals') or 0, ds.get('extrema') or 0, ds.get('sections_x'), ds.get('sections_y'))

    # -- domain series ----------------------------------------------------------
    def _domain_series_refusal(self):
        if self._gp_models or self.input.get('gp') is not None:
            raise NotImplementedError("domain series: surrogate (GP) closures replace the pressure and wall stress the series evaluate, "
                                      "and a slab with surrogates steps stage-wise (not supported)")
        if self._thinning:
            raise NotImplementedError("domain series: shear thinning needs grad p and steps stage-wise on slabs (not supported)")
        if self._elastic is not None:
            raise NotImplementedError("domain series: an elastic gap steps stage-wise on slabs and deforms between steps (not supported)")
        if self.driver.p2p:
            raise NotImplementedError("domain series: not recorded over the peer-to-peer transport (its batches have no host between steps); "
                                      "arm them on the all-gather transport")

    def set_domain_series(self, integrals=0, extrema=0, sections_x=None, sections_y=None):
        """Record, over the WHOLE domain and on every rank, the film integrals after every step whose count is a multiple of
        `integrals` and the field extrema after every multiple of `extrema` (strides; 0: that series is off): the records of
        Problem.set_integrals / Problem.set_extrema, bit for bit what the undivided problem records for the same state.
        sections_x / sections_y: up to 8 GLOBAL 1-based interior rows / columns of the flow sections, default the first and last of
        the domain, as on a Problem.  Each rank reduces its own rows on the device; one all-gather of 32 doubles per row carries
        them, and every rank folds all rows in the undivided order (csrc/slab_series_kernels.hip), so every rank holds the same
        series.  Collective: the same arguments on every rank.  Starts new series (``domain_integrals``, ``domain_extrema``).
        While armed, steps are enqueued eagerly even with GPF_SLAB_GRAPH=1.  Not available with surrogate closures, shear
        thinning or an elastic gap (these slabs step stage-wise), nor over the peer-to-peer transport.  Checkpoints do not carry
        the series: a slab restored from one whose options hold `domain_series` has them armed again and its series start
        empty."""
        self._domain_series_refusal()
        d = _domain_series_entry({'integrals': integrals, 'extrema': extrema, 'sections_x': sections_x, 'sections_y': sections_y},
                                 self.grid['Nx'], self.grid['Ny'])
        if not d['integrals'] and not d['extrema']:
            raise ValueError("domain series: at least one of the strides `integrals`, `extrema` must be >= 1 (clear_domain_series disarms)")
        sx = _integral_sections(d['sections_x'], self.grid['Nx'], 'sections_x')
        sy = _integral_sections(d['sections_y'], self.grid['Ny'], 'sections_y')
        self.driver.series = None
        self.driver.series = self._domain = _DomainSeries(self, d['integrals'], d['extrema'], sx, sy)

    def clear_domain_series(self):
        """Stop recording and free the device buffers.  Collective."""
        if self._domain is not None:
            self._domain.clear()
        self.driver.series = self._domain = None

    @property
    def domain_integrals(self):
        """FilmIntegrals of the whole domain -- the keys, shapes and dtypes of Problem.integrals -- of every recorded step since
        set_domain_series (or pre_run), across advance() / run() calls; the same on every rank.  None while not armed."""
        if self._domain is None or self._domain.film is None:
            return None
        from .problem import _film_series
        return _film_series(self._domain.film, *self._domain.sections)

    @property
    def domain_extrema(self):
        """FieldExtrema of the whole domain -- as Problem.extrema, the cells' ix global in the ghosted index space -- of every
        recorded step since set_domain_series (or pre_run); the same on every rank.  None while not armed."""
        if self._domain is None or self._domain.ext is None:
            return None
        from .problem import _extrema_series
        return _extrema_series(self._domain.ext)

    def _domain_now(self):
        self._domain_series_refusal()
        d = self._domain
        if d is not None:
            return d, d.now(self.dist)
        sx = _integral_sections(None, self.grid['Nx'], 'sections_x')        # not armed: the default sections, as on a Problem
        sy = _integral_sections(None, self.grid['Ny'], 'sections_y')
        d = _DomainSeries(self, 0, 0, sx, sy)
        try:
            return d, d.now(self.dist)
        finally:
            d.clear()

    def domain_film_integrals(self):
        """Problem.film_integrals for the whole domain: the record of the current state, as a dict of the names of
        ``domain_integrals``.  Armed or not (then with the default sections).  Collective; the same dict on every rank."""
        d, (out, _, _) = self._domain_now()
        sx, sy = d.sections
        ns = len(_lib.INTEGRAL_SUMS)
        res = {name: np.float64(out[k]) for k, name in enumerate(_lib.INTEGRAL_SUMS)}
        res.update(flow_x=out[ns:ns + len(sx)].copy(), flow_y=out[ns + len(sx):].copy(),
                   sections_x=np.array(sx, dtype=np.int64), sections_y=np.array(sy, dtype=np.int64))
        return res

    def domain_field_extrema(self):
        """Problem.field_extrema for the whole domain: the seven names of ``domain_extrema`` and, for each, `<name>_cell` =
        (ix, iy), ix global.  Armed or not.  Collective; the same dict on every rank."""
        _, (_, vals, cells) = self._domain_now()
        res = {}
        for k, name in enumerate(_lib.EXTREMA_NAMES):
            res[name] = np.float64(vals[k])
            res[name + '_cell'] = (int(cells[k, 0]), int(cells[k, 1]))
        return res

    def _shared_asperity_heights(self, geo):
        """topography.py:141-146 draws the minimum heights of num^2 asperities from an unseeded normal distribution: every
        rank must use rank 0's draw."""
        if geo['type'] != 'asperity' or geo['num'] == 1:
            return None
        h0, h1, num = geo['hmin'], geo['hmax'], geo['num']
        box = [np.random.normal(loc=h0 + (h1 - h0) / 2., scale=(h1 - h0) / 2. / 2.57, size=num**2) if self.rank == 0 else None]
        self.dist.broadcast_object_list(box, src=0)
        return box[0]

    def connect_p2p(self):
        """Switch the fused slab step to the peer-to-peer transport (ranks of one node): exchange the mailboxes'
        IPC handles once through the process group, map them, and from then on `advance` enqueues whole batches of
        steps whose kernels talk to each other directly.  Collective; returns False (and stays on the all-gather
        transport) unless every rank succeeded."""
        if getattr(self, '_domain', None) is not None:
            raise NotImplementedError("domain series: not recorded over the peer-to-peer transport; clear_domain_series first")
        t, L = self.torch, self.layout
        buf = (C.c_ubyte * 64)()
        ok = self.lib.gpf_p2p_export(self._h, buf, 64) == 0
        mine = t.tensor(list(buf), dtype=t.uint8).to('cuda')
        everyone = t.zeros(64 * self.world, dtype=t.uint8, device='cuda')
        self.dist.all_gather_into_tensor(everyone, mine)
        if ok:
            handles = everyone.cpu().numpy().tobytes()
            d = self.driver
            ok = self.lib.gpf_p2p_connect(self._h, self.rank, self.world, handles, d.rank_lo, d.rank_hi) == 0
        if not ok:
            print(f"[gapflow_amd] rank {self.rank}: peer-to-peer transport unavailable: "
                  f"{self.lib.gpf_last_error().decode()}", file=sys.stderr)
        flag = t.tensor([1.0 if ok else 0.0], dtype=t.float64, device='cuda')
        self.dist.all_reduce(flag, op=self.dist.ReduceOp.MIN)
        self.driver.p2p = bool(flag.item() == 1.0)
        return self.driver.p2p

    def __del__(self):
        h = getattr(self, '_h', None)
        if h is not None and h.value:
            self.lib.gpf_destroy(h)
            h.value = None

    @classmethod
    def from_string(cls, text, device=0, dist=None, base_dir=None):
        from .problem import _keep_own_options
        with _io.StringIO(text) as f:
            d = read_yaml_input(f)
        _keep_own_options(d, text, base_dir)        # options.checkpoint_freq, as Problem.from_string; the series' keys: refused in __init__, but domain_series
        return cls(d, device=device, dist=dist)

    @classmethod
    def from_yaml(cls, fname, device=0):
        with open(fname) as f:
            return cls.from_string(f.read(), device=device, base_dir=os.path.dirname(os.path.abspath(fname)))

    def _upload(self, field, arr):
        a = _lib.f64c(arr)
        _lib.check(self.lib.gpf_upload(self._h, field, _lib.as_dp(a), a.size))

    # -- checkpoint and restart -------------------------------------------------
    def _checkpoint_refusal(self):
        from .checkpoint import NOT_SAVED
        if self._gp_models or self.input.get('gp') is not None:
            raise NotImplementedError(NOT_SAVED['surrogate'])
        if self._elastic is not None:
            raise NotImplementedError(NOT_SAVED['elastic slab'])
        geo = self.input['geometry']
        if geo['type'] == 'asperity' and geo['num'] != 1:
            # the seam rows and the writer's gap are rebuilt from the YAML, and these heights are an unseeded random draw
            raise NotImplementedError(NOT_SAVED['random asperities on slabs'])
        if not self._pre_run_done:
            raise RuntimeError("checkpoint: call pre_run() (or run()) first")

    def save_checkpoint(self, path):
        """Every rank writes its own rows into ``path.rankNNN`` (atomically, as Problem.save_checkpoint); rank 0's file also
        carries the history of the output frames.  Collective only in that every rank has to call it at the same step."""
        from . import checkpoint
        self._checkpoint_refusal()
        self.torch.cuda.current_stream().synchronize()
        d = self.input
        meta = {'kind': 'slab', 'world': self.world, 'rank': self.rank,
                'inputs': checkpoint.input_dicts(d['options'], d['grid'], d['numerics'], d['properties'], d['geometry'])}
        if self.rank == 0:
            w = self._writer_problem
            meta['mirror'] = {'history': w.history if w is not None else (self._restart_history or {})}
        checkpoint.write_file(checkpoint.rank_path(path, self.rank), meta, checkpoint.device_blob(self.lib, self._h))

    def _write_checkpoint(self):
        """checkpoint.gpf.rankNNN in rank 0's output directory (every rank learns its name from rank 0)."""
        box = [self._writer_problem.outdir if self.rank == 0 else None]
        self.dist.broadcast_object_list(box, src=0)
        self.save_checkpoint(os.path.join(box[0], 'checkpoint.gpf'))

    def load_checkpoint(self, path):
        """This rank's file of a save on the same number of ranks, into this problem (after pre_run).  The all-gather transport
        only: a problem connected for the peer-to-peer transport refuses (its mailboxes' sequence numbers cannot be put back)."""
        from . import checkpoint
        self._checkpoint_refusal()
        try:
            meta, blob = checkpoint.read_file(checkpoint.rank_path(path, self.rank))
        except ValueError as e:
            raise RuntimeError(str(e)) from None
        if meta.get('kind') != 'slab' or meta.get('world') != self.world or meta.get('rank') != self.rank:
            raise RuntimeError(f"checkpoint: {checkpoint.rank_path(path, self.rank)} was written by rank {meta.get('rank')} of "
                               f"{meta.get('world')} (kind '{meta.get('kind')}'); this is rank {self.rank} of {self.world}")
        self.torch.cuda.current_stream().synchronize()
        checkpoint.load_device_blob(self.lib, self._h, blob)
        st = self.state()
        self.driver.enqueued = int(st.step)         # the sweep direction of a captured pair of steps follows it
        self.driver.graph = None
        self._closures_stale = True
        if self.rank == 0:
            self._restart_history = {k: list(v) for k, v in (meta.get('mirror', {}).get('history') or {}).items()} or None

    @classmethod
    def from_checkpoint(cls, path, device=0, dist=None, options=None, numerics=None):
        """A new slab problem on every rank that continues the saved one; the process group must have the world size of the save."""
        from . import checkpoint
        if dist is None:
            import torch.distributed as dist
        rank, world = dist.get_rank(), dist.get_world_size()
        first = checkpoint.rank_path(path, rank)
        if not os.path.exists(first):
            raise RuntimeError(f"checkpoint: {first} not found: a slab checkpoint loads on the world size it was written on "
                               f"(this one: {world})")
        try:
            meta, _ = checkpoint.read_file(first)
        except ValueError as e:
            raise RuntimeError(str(e)) from None
        if meta.get('world') != world:
            raise RuntimeError(f"checkpoint: written on {meta.get('world')} ranks, this process group has {world}")
        inp = meta['inputs']
        for given, allowed, target in ((options, ('output', 'silent', 'use_tstamp', 'write_freq'), inp['options']),
                                       (numerics, ('max_it', 'tol'), inp['numerics'])):
            for k, v in (given or {}).items():
                if k not in allowed:
                    raise ValueError(f"from_checkpoint: '{k}' cannot be overridden (only {allowed})")
                target[k] = v
        p = cls(inp, device=device, dist=dist)
        p.pre_run()
        p.load_checkpoint(path)
        return p

    def global_scalars(self):
        """Ekin, v_max, v_sound, mass over the whole domain (sum / max over the slabs)."""
        sc = _lib.GpfScalars()
        _lib.check(self.lib.gpf_scalars(self._h, C.byref(sc)))
        t = self.torch
        s = t.tensor([sc.ekin, sc.mass], dtype=t.float64, device='cuda')
        m = t.tensor([sc.v_max, sc.v_sound], dtype=t.float64, device='cuda')
        self.dist.all_reduce(s, op=self.dist.ReduceOp.SUM)
        self.dist.all_reduce(m, op=self.dist.ReduceOp.MAX)
        return {'ekin': float(s[0]), 'mass': float(s[1]), 'v_max': float(m[0]), 'v_sound': float(m[1])}

    # -- what a SlabSurrogate asks of its problem -----------------------------------------------
    def _download(self, field, ncomp):
        out = np.empty((ncomp,) + self._shape)
        _lib.check(self.lib.gpf_download(self._h, field, _lib.as_dp(out), out.size))
        return out

    def _sync_to_device(self):
        pass

    def _gather_pairs(self, value, payload):
        t = self.torch
        self._pair.copy_(t.tensor([value] + list(payload), dtype=t.float64))
        self.dist.all_gather_into_tensor(self._pairs, self._pair)
        return self._pairs.cpu().numpy().reshape(self.world, 8)

    def domain_max(self, value):
        return float(np.max(self._gather_pairs(value, np.zeros(7))[:, 0]))

    def features_of_domain_max(self, value, features):
        """Feature row of the most uncertain cell of the whole domain: the lowest rank holding the maximum wins,
        like the first hit of the serial argmax (rows shared by two slabs carry identical features)."""
        pairs = self._gather_pairs(value, features)
        return pairs[int(np.argmax(pairs[:, 0])), 1:].copy()

    def _features_local(self):
        topo = self._topo_local if self._elastic is None else self._download(_lib.FIELD_TOPO, 3)
        return np.vstack([self.local_q(), topo, self._extra]).reshape(7, -1).T

    def pre_run(self):
        """Problem._pre_run (problem.py:412-443) with domain-wide scalars."""
        if self._gp_models:
            self.database.initialize(self._features_global, self.grid['dim'])       # identical on every rank
            for m in self._gp_models.values():
                m.init()
        _lib.check(self.lib.gpf_pre_run(self._h))
        g = self.global_scalars()
        num, grid = self.input['numerics'], self.input['grid']
        dt_crit = min(grid['dx'], grid['dy']) / (g['v_max'] + g['v_sound'])
        dt = num['CFL'] * dt_crit if num['adaptive'] else num['dt']
        _lib.check(self.lib.gpf_set_dt(self._h, float(dt)))
        _lib.check(self.lib.gpf_set_ekin_old(self._h, float(g['ekin'])))
        self._pre_run_done = True
        if self._domain is not None:
            self._domain.reset()                # the step count starts over: so do the domain series

    def advance(self, n, honor_stop=False, write_freq=None):
        if not self._gp_models and not self._thinning and self._elastic is None:
            return self.driver.advance(n, honor_stop)
        for _ in range(n):
            st = self.state()
            if st.invalid or (honor_stop and (st.converged or st.step >= self.input['numerics']['max_it'])):
                break
            self._stagewise_step(write_freq or self.input['options']['write_freq'], st.step)

    def _stagewise_step(self, write_freq, step):
        """Problem._update_with_surrogates for a slab: the working field's outer rows travel after each stage
        (the closures of the next stage read them), the scalar records once at the end."""
        lib, h, d = self.lib, self._h, self.driver
        gathered = C.c_void_p(d.gathered.data_ptr())
        one_step_before_output = (step + 1) % write_freq == 0
        feats = None

        def features_of_cell(i):
            nonlocal feats
            if feats is None:
                feats = self._features_local()
            return feats[i]

        _lib.check(lib.gpf_open_step(h))
        for i in range(2):
            for m in self._gp_models.values():
                m.sync_scales()
            _lib.check(lib.gpf_stage_closures(h))
            changed = False
            for name in ('zz', 'xz', 'yz'):
                m = self._gp_models.get(name)
                if m is not None:
                    changed |= m.stage(i == 0, one_step_before_output, features_of_cell)
            if changed:
                _lib.check(lib.gpf_stage_closures(h))
            _lib.check(lib.gpf_stage_advance(h, i))
            _lib.check(lib.gpf_stage_message(h))
            self.dist.all_gather_into_tensor(d.gathered, d.message)
            _lib.check(lib.gpf_stage_absorb(h, gathered, self.world, d.rank_lo, d.rank_hi))
        for m in self._gp_models.values():
            m.sync_scales()
        _lib.check(lib.gpf_close_step_local(h))
        self.dist.all_gather_into_tensor(d.gathered, d.message)
        sc = _lib.GpfScalars()
        _lib.check(lib.gpf_close_step_commit(h, gathered, self.world, C.byref(sc)))
        if self._elastic is not None and not sc.invalid:
            # Topography.update (problem.py:566) with the pressure of the corrector's closures; the record all-gather above
            # carried p_ref; sc.invalid is the same on every rank (rank-ordered reduction)
            self._elastic.step(gathered)
        return sc

    def state(self):
        sc = _lib.GpfScalars()
        _lib.check(self.lib.gpf_state(self._h, C.byref(sc)))
        if sc.invalid == 3:
            raise RuntimeError("slab step: a peer rank did not deliver its rows within 30 s (peer-to-peer transport)")
        return sc

    # -- Problem.run for slabs -----------------------------------------------------------------
    def gather_q(self):
        """The whole field (3, Nx+2, Ny+2) on every rank: owned rows from their owners, the domain's two ghost rows
        from the first and last rank.  Collective; meant for output frames, not for the time loop."""
        return self._gather_rows(self.local_q())

    def gather_topo(self):
        """The whole deformed gap (4, Nx+2, Ny+2): h, dh/dx, dh/dy, displacement, gathered like gather_q."""
        local = np.concatenate([self._download(_lib.FIELD_TOPO, 3), self._download(_lib.FIELD_DEFORMATION, 1)])
        return self._gather_rows(local)

    def _gather_rows(self, local):
        t, L = self.torch, self.layout
        parts = partition(L.Nx_global, self.world)
        max_nx = max(hi - lo + 1 for lo, hi in parts)
        ny2, nc = self._shape[1], local.shape[0]
        mine = np.zeros((nc, max_nx + 2, ny2))
        mine[:, :L.nx + 2] = local
        send = t.from_numpy(mine.reshape(-1)).to('cuda')
        recv = t.zeros(send.numel() * self.world, dtype=t.float64, device='cuda')
        self.dist.all_gather_into_tensor(recv, send)
        allq = recv.cpu().numpy().reshape(self.world, nc, max_nx + 2, ny2)
        out = np.empty((nc, L.Nx_global + 2, ny2))
        for r, (lo, hi) in enumerate(parts):
            out[:, lo:hi + 1] = allq[r, :, 1:hi - lo + 2]
        out[:, 0] = allq[0, :, 0]
        out[:, -1] = allq[-1, :, parts[-1][1] - parts[-1][0] + 2]
        return out

    def _frame(self):
        """One output frame through a whole-domain Problem that only rank 0 holds: it owns the output directory, the
        NetCDF / csv writers and the closures of the frame (Problem.write, problem.py:616-637)."""
        q = self.gather_q()
        topo = self.gather_topo() if self._elastic is not None else None
        if self.rank != 0:
            return
        if self._writer_problem is None:
            from .problem import Problem
            d = deepcopy(self.input)
            d['options'].pop('frames', None)        # stored, never armed: the writer steps nothing, and frames are not recorded on slabs
            d['options'].pop('thinning_series', None)       # likewise the thinning series
            # with surrogates the writer shares this rank's database and mirrors its models (same data, same
            # hyper-parameters), so the closures of a frame are the surrogates' means as in a serial run
            self._writer_problem = Problem(d['options'], d['grid'], d['numerics'], d['properties'], d['geometry'],
                                           gp=d.get('gp') if self._gp_models else None,
                                           database=self.database if self._gp_models else None, device=self._device,
                                           elastic_on_device=False)
            w = self._writer_problem
            w.history = self._restart_history or {k: [] for k in ('step', 'time', 'ekin', 'residual', 'vsound')}
        w = self._writer_problem
        for name, m in self._gp_models.items():
            wm = w._gp_models[name]
            if wm.theta is None or wm.last_fit_train_size != m.last_fit_train_size or not np.array_equal(wm.theta, m.theta):
                wm.theta, wm.last_fit_train_size = np.array(m.theta), m.last_fit_train_size
                wm.attach()
        if topo is not None:            # the deformed gap of the slabs: topo.nc's frame and the frame's closures
            w.topo.full[...] = topo
            w._upload_topo()
        st = self.state()
        w.q[...] = q
        w.step, w.simtime, w.dt, w.residual = int(st.step), st.simtime, st.dt, st.residual
        # (a restarted run's history already ends with the row of the step it starts from)
        w.write(scalars=not (w.history['step'] and w.history['step'][-1] == w.step), params=False)

    def run(self):
        """Problem.run (problem.py:368-410) for a slab-decomposed problem: same stopping rules (tolerance on the last
        five residuals, max_it, invalid state), same status lines and output files, written by rank 0."""
        import datetime as _dt
        opt, num = self.input['options'], self.input['numerics']
        silent, wf, max_it = opt['silent'], opt['write_freq'], num['max_it']
        cf = 0 if silent else int(opt.get('checkpoint_freq', 0) or 0)        # steps between checkpoints; 0: none
        if not self._pre_run_done:
            self.pre_run()
        if not silent:
            if self.rank == 0:
                print(61 * '-')
                print(f"{'Step':6s} {'Timestep':10s} {'Time':10s} {'CFL':10s} {'Residual':10s}")
                print(61 * '-')
            self._frame()
        tic = _dt.datetime.now()
        st = self.state()
        while not st.converged and st.step < max_it and not st.invalid:
            n = min(wf - st.step % wf, max_it - st.step, 4096, *([cf - st.step % cf] if cf > 0 else []))
            self.advance(n, honor_stop=True)
            st = self.state()
            if st.invalid:
                if self.rank == 0:
                    print('NaN detected.' if st.invalid == 1 else 'Negative density detected.',
                          'Writing previous step and aborting simulation.')
                break
            if st.step % wf == 0 and not silent:
                self._frame()
            if cf > 0 and st.step % cf == 0 and not st.converged and st.step < max_it:
                self._write_checkpoint()
        if not silent and st.step % wf != 0:
            self._frame()
        if cf > 0 and not st.invalid:
            self._write_checkpoint()            # the state the run ends on
        if self.rank == 0:
            wall = _dt.datetime.now() - tic
            print(33 * '=')
            print("Total walltime   : ", str(wall).split('.')[0])
            print(f"({st.step / max(wall.total_seconds(), 1e-12):.2f} steps/s)")
            print(33 * '=')
            if not silent:
                from .io import history_to_csv
                w = self._writer_problem
                w._writer.close()
                history_to_csv(os.path.join(w.outdir, 'history.csv'), w.history)
                from .problem import _save_extrema_series, _save_film_series
                if self.domain_integrals is not None:       # the files a serial run with options.integrals / options.extrema writes
                    _save_film_series(w.outdir, self.domain_integrals)
                if self.domain_extrema is not None:
                    _save_extrema_series(w.outdir, self.domain_extrema)
        return st

    def local_q(self):
        out = np.empty((3,) + self._shape)
        _lib.check(self.lib.gpf_download(self._h, _lib.FIELD_Q, _lib.as_dp(out), out.size))
        return out


class SlabElastic:
    """Elastic deformation of the gap on an x-slab: the distributed half-space convolution (gapflow_amd/elastic.py:
    SlabElasticPlan, csrc/api_slab_elastic.inc) and its collectives -- two uneven all-to-alls and, unless the half-space
    is fully periodic, an all-gather of 8 doubles that hands rank 0's reference displacement to every rank."""

    def __init__(self, slab, grid, el, topo_rows):
        from .elastic import ElasticDeformation, SlabElasticPlan
        self.slab, torch, lib, h = slab, slab.torch, slab.lib, slab._h
        self.host = ElasticDeformation(el['E'], el['v'], el['alpha_underrelax'], grid, el['n_images'])
        self.plan = P = SlabElasticPlan.for_grid(grid, slab.world, self.host.shape_fft)
        r = slab.rank
        h0 = topo_rows(P.return_rows(r))[0]
        self.host.attach_slab(slab, P, r, h0)
        self.relative = self.host.periodicity != 'full'

        def buf(which):
            p, n = C.c_void_p(), C.c_size_t(0)
            _lib.check(lib.gpf_elastic_slab_buffer(h, which, C.byref(p), C.byref(n)))
            if n.value == 0:
                return torch.empty(0, dtype=torch.float64, device='cuda')
            return torch.as_tensor(_DeviceArray(p.value, n.value), device='cuda')
        self.send1, self.recv1, self.send2, self.recv2, self.ref, self.refs = (buf(i) for i in range(6))
        two = lambda counts: [2 * c for c in counts]          # complex numbers -> doubles
        self.splits1 = (two(P.recv1(r)), two(P.send1(r)))
        self.splits2 = (two(P.recv2(r)), two(P.send2(r)))

    def step(self, gathered):
        s = self.slab
        lib, h, dist = s.lib, s._h, s.dist
        _lib.check(lib.gpf_elastic_slab_forward(h, gathered, s.world))
        dist.all_to_all_single(self.recv1, self.send1, *self.splits1)
        _lib.check(lib.gpf_elastic_slab_convolve(h))
        dist.all_to_all_single(self.recv2, self.send2, *self.splits2)
        _lib.check(lib.gpf_elastic_slab_finish(h))
        if self.relative:
            dist.all_gather_into_tensor(self.refs, self.ref)
        _lib.check(lib.gpf_elastic_slab_apply(h))
