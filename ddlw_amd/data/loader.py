"""Sharded streaming Parquet loader — the Petastorm-converter equivalent.

Reference contract (SURVEY.md §2.5 Petastorm row;
``Part 1 .../03_model_training_distributed.py:135-144, 197-234, 332-337``):

- ``make_converter(df_or_table)`` materialises the table into a Parquet cache
  dir and returns a converter; ``len(converter)`` = row count (:143-144);
- ``converter.make_torch_dataset(batch_size, cur_shard, shard_count)`` is a
  context manager yielding an *infinite* batch stream (``num_epochs=None``
  semantics, :199) sharded per rank;
- ``converter.delete()`` removes the cache (:425-426).

MI355X-native design (not a Petastorm port):

- sharding is by Parquet **row group**: rank r owns row groups
  r, r+W, r+2W, ... of the dataset (disjoint + exhaustive across ranks),
  cycled infinitely — tested in ``tests/test_loader.py``;
- a CPU worker pool decodes/praeprocesses JPEG rows into batch tensors;
- on GPU, batches are staged through **pinned host buffers** and copied with
  ``hipMemcpyAsync`` on a **side HIP stream** (``torch.cuda.Stream``), double
  buffered so H2D overlaps compute; the consumer stream waits on a recorded
  event, never the host.
"""
from __future__ import annotations

import heapq
import itertools
import queue
import threading
import uuid
from collections import deque
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path
from typing import Callable, Iterator, List, Optional, Tuple

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq
import torch

from .preprocess import preprocess_bytes
from ..core.config import current_setup


def _default_transform(content, img_height: int, img_width: int):
    # module-level (picklable) so the decode pool can use forkserver
    return preprocess_bytes(content, img_height, img_width)


def _uint8_transform(content, img_height: int, img_width: int):
    # ``output="uint8"``: HWC uint8, normalization left to the device.
    # Module-level (picklable) like the default; decode.py imports this
    # module, hence the import here.
    from .decode import decode_resize_u8

    return torch.from_numpy(np.array(decode_resize_u8(content, img_height, img_width)))


_forkserver_preloaded = False


def _pool_ctx(transform):
    """Start-method choice for the decode pool. Plain fork of a
    CUDA-initialized parent can wedge the child (forked while another
    thread holds a runtime/allocator lock) — children then sit ALIVE but
    dead, observed as a silent hang late in big GPU test sessions. When
    CUDA is up and the transform is picklable, use a forkserver (workers
    fork from a small clean server; the server preloads this module once
    so each worker skips the torch import)."""
    import multiprocessing as mp
    import pickle

    try:
        cuda_up = torch.cuda.is_initialized()
    except Exception:
        cuda_up = False
    if cuda_up and "forkserver" in mp.get_all_start_methods():
        try:
            pickle.dumps(transform)
            ctx = mp.get_context("forkserver")
            global _forkserver_preloaded
            if not _forkserver_preloaded:
                ctx.set_forkserver_preload(["ddlw_amd.data.loader"])
                _forkserver_preloaded = True
            return ctx
        except Exception:
            pass
    method = "fork" if "fork" in mp.get_all_start_methods() else "spawn"
    return mp.get_context(method)


def shard_row_groups(num_row_groups: int, cur_shard: int, shard_count: int) -> List[int]:
    """Row groups owned by shard ``cur_shard`` of ``shard_count``:
    disjoint across shards, exhaustive, round-robin (rank r gets r, r+W, ...)."""
    if not (0 <= cur_shard < shard_count):
        raise ValueError(f"cur_shard {cur_shard} out of range for {shard_count}")
    return list(range(cur_shard, num_row_groups, shard_count))


def _decode_worker(transform, shm_name, view_shape, dtype_str, task_q, res_q):
    """Decode-pool worker: pull (seq, slot, [jpeg bytes...]) tasks, decode
    each image with ``transform`` straight into shared-memory slot ``slot``,
    report (status, seq, slot, n). Decoded pixels never cross a pipe."""
    from multiprocessing import shared_memory

    shm = shared_memory.SharedMemory(name=shm_name)
    view = np.ndarray(view_shape, dtype=np.dtype(dtype_str), buffer=shm.buf)
    try:
        while True:
            task = task_q.get()
            if task is None:
                return
            seq, slot, chunk = task
            try:
                for i, c in enumerate(chunk):
                    out = transform(c)
                    if isinstance(out, torch.Tensor):
                        out = out.numpy()
                    view[slot, i] = out
                res_q.put(("ok", seq, slot, len(chunk)))
            except Exception as e:  # surfaced in the main process
                res_q.put(("err", seq, slot, repr(e)))
    finally:
        shm.close()
        # flush the result queue's feeder thread, then hard-exit: a forked
        # child of a HIP-initialized parent must NOT run the inherited HIP
        # atexit handlers (they touch runtime state owned by the parent and
        # can crash the child at teardown)
        try:
            res_q.close()
            res_q.join_thread()
        except Exception:
            pass
        import os as _os

        _os._exit(0)


class _ProcDecodePool:
    """Process-based JPEG decode pool over a shared-memory slot ring.

    The GIL makes a thread pool top out near single-core decode throughput
    (round-1 measured 1,240 img/s with 96 threads vs a 8,900 img/s GPU step);
    real parallel decode needs processes. Workers are forked (the transform
    callable is inherited, no pickling) and write decoded images directly
    into /dev/shm slots sized one batch each; the main process only ships
    jpeg bytes in and slot indices out, then memcpys slot -> pinned buffer
    (GIL released) for the side-stream H2D. Petastorm's reader-pool
    equivalent (reference P1/03:199-200)."""

    SHM_CAP_BYTES = 8 << 30  # ring cap; also caps in-flight parallelism

    def __init__(self, transform, sample_shape, sample_dtype, batch_size: int,
                 workers: int, pin: bool = False):
        from multiprocessing import shared_memory

        ctx = _pool_ctx(transform)
        self.workers = max(1, int(workers))
        self.slot_shape = (int(batch_size),) + tuple(int(s) for s in sample_shape)
        self.np_dtype = np.dtype(sample_dtype)
        slot_bytes = int(np.prod(self.slot_shape)) * self.np_dtype.itemsize
        self.slots = max(2, min(self.workers + 2,
                                self.SHM_CAP_BYTES // max(slot_bytes, 1)))
        self.shm = shared_memory.SharedMemory(
            create=True, size=max(slot_bytes * self.slots, 1))
        view_shape = (self.slots,) + self.slot_shape
        self.view = np.ndarray(view_shape, dtype=self.np_dtype, buffer=self.shm.buf)
        # Pin the ring: the shm pages are MAP_SHARED, i.e. the SAME physical
        # pages the forked workers write — hipHostRegister-ing the parent's
        # mapping makes every slot DMA-able, so H2D copies run straight from
        # the decode output with no staging memcpy.
        self.pinned = False
        if pin:
            try:
                r = torch.cuda.cudart().cudaHostRegister(
                    int(self.view.ctypes.data), int(self.shm.size), 0)
                self.pinned = (int(r) == 0)
            except Exception:
                self.pinned = False
        self.task_q = ctx.Queue()
        self.res_q = ctx.Queue()
        self.procs = [
            ctx.Process(
                target=_decode_worker,
                args=(transform, self.shm.name, view_shape, self.np_dtype.str,
                      self.task_q, self.res_q),
                daemon=True,
            )
            for _ in range(self.workers)
        ]
        for p in self.procs:
            p.start()

    def any_dead(self) -> List[int]:
        return [p.pid for p in self.procs if not p.is_alive()]

    def close(self) -> None:
        for _ in self.procs:
            try:
                self.task_q.put_nowait(None)
            except Exception:
                pass
        for p in self.procs:
            p.join(timeout=2.0)
        for p in self.procs:
            if p.is_alive():
                p.terminate()
                p.join(timeout=2.0)
        for q_ in (self.task_q, self.res_q):
            try:
                q_.close()
                q_.cancel_join_thread()
            except Exception:
                pass
        if self.pinned:
            try:
                torch.cuda.cudart().cudaHostUnregister(int(self.view.ctypes.data))
            except Exception:
                pass
            self.pinned = False
        try:
            self.shm.close()
            self.shm.unlink()
        except Exception:
            pass


class _H2DStager:
    """Pinned-buffer + side-stream H2D pipeline (double buffered)."""

    def __init__(self, device: torch.device, depth: int = 2):
        self.device = device
        self.stream = torch.cuda.Stream(device=device)
        self.depth = depth
        self._pinned: List[Tuple[torch.Tensor, torch.Tensor]] = []
        self._slot = 0

    def stage(self, images: torch.Tensor, labels: torch.Tensor):
        """Copy a CPU batch to the device on the side stream; returns device
        tensors + an event the consumer stream must wait on."""
        if not self._pinned or self._pinned[0][0].shape != images.shape:
            self._pinned = [
                (
                    torch.empty_like(images, pin_memory=True),
                    torch.empty_like(labels, pin_memory=True),
                )
                for _ in range(self.depth)
            ]
            self._events = [torch.cuda.Event() for _ in range(self.depth)]
            self._slot = 0
        slot = self._slot
        self._slot = (self._slot + 1) % self.depth
        pi, pl = self._pinned[slot]
        ev = self._events[slot]
        # don't overwrite a pinned buffer still being read by an in-flight copy
        ev.synchronize()
        pi.copy_(images)
        pl.copy_(labels)
        with torch.cuda.stream(self.stream):
            di = pi.to(self.device, non_blocking=True)
            dl = pl.to(self.device, non_blocking=True)
            ev.record(self.stream)
        return di, dl, ev


class ShardedParquetLoader:
    """Iterates (images, labels) batches from a Parquet dataset shard.

    ``output="float"`` (default): fp32 N x C x H x W in [-1, 1].
    ``output="uint8"``: the decoded bytes, N x H x W x C — a quarter of the
    H2D traffic; the normalize then belongs to the model
    (``train.Model(precision="bf16")`` takes these batches as they are).
    A custom ``transform=`` replaces either and excludes ``output="uint8"``."""

    def __init__(
        self,
        dataset_path: str,
        batch_size: int = 32,
        cur_shard: int = 0,
        shard_count: int = 1,
        img_height: int = 224,
        img_width: int = 224,
        num_epochs: Optional[int] = None,  # None = infinite (Petastorm default)
        workers: int = 4,
        device: Optional[torch.device] = None,
        content_column: str = "content",
        label_column: str = "label_idx",
        transform: Optional[Callable] = None,
        prefetch: int = 2,
        pool: str = "auto",  # "process" | "thread" | "auto"
        output: str = "float",  # "float": fp32 CHW in [-1, 1] | "uint8": HWC bytes
    ):
        self.path = str(dataset_path)
        self.files = sorted(str(p) for p in Path(self.path).glob("*.parquet")) or [self.path]
        self.batch_size = batch_size
        self.cur_shard = cur_shard
        self.shard_count = shard_count
        self.img_height = img_height
        self.img_width = img_width
        self.num_epochs = num_epochs
        self.workers = workers
        self.device = device
        self.content_column = content_column
        self.label_column = label_column
        import functools

        if output not in ("float", "uint8"):
            raise ValueError(f"output must be float|uint8, got {output!r}")
        if transform is not None and output == "uint8":
            raise ValueError(
                "transform= and output='uint8' both choose the decode step; "
                "give one of them")
        self.output = output
        self.transform = transform or functools.partial(
            _uint8_transform if output == "uint8" else _default_transform,
            img_height=self.img_height, img_width=self.img_width)
        self.prefetch = prefetch
        if pool not in ("auto", "process", "thread"):
            raise ValueError(f"pool must be auto|process|thread, got {pool!r}")
        self.pool = pool
        # (file_idx, row_group_idx) pairs across all files
        self._rg_index: List[Tuple[int, int]] = []
        self._num_rows = 0
        for fi, f in enumerate(self.files):
            md = pq.ParquetFile(f).metadata
            self._num_rows += md.num_rows
            for g in range(md.num_row_groups):
                self._rg_index.append((fi, g))
        self._stager = None

    def __len__(self) -> int:
        return self._num_rows

    # ------------------------------------------------------------------ #
    def _shard_groups(self) -> List[Tuple[int, int]]:
        idx = shard_row_groups(len(self._rg_index), self.cur_shard, self.shard_count)
        return [self._rg_index[i] for i in idx]

    def _iter_rows(self) -> Iterator[Tuple[bytes, int]]:
        readers = {fi: pq.ParquetFile(f) for fi, f in enumerate(self.files)}
        if len(self._rg_index) >= self.shard_count:
            groups = self._shard_groups()
            row_filter = None
        else:
            # fewer row groups than ranks: fall back to row-level round-robin
            # so every rank still gets a non-empty, disjoint, exhaustive shard
            groups = list(self._rg_index)
            row_filter = (self.cur_shard, self.shard_count)
        if not groups:
            return
        epoch = 0
        while self.num_epochs is None or epoch < self.num_epochs:
            row_idx = 0
            for fi, g in groups:
                tbl = readers[fi].read_row_group(g, columns=[self.content_column, self.label_column])
                contents = tbl.column(self.content_column).to_pylist()
                labels = tbl.column(self.label_column).to_pylist()
                for c, l in zip(contents, labels):
                    if row_filter is None or row_idx % row_filter[1] == row_filter[0]:
                        yield c, l
                    row_idx += 1
            epoch += 1

    def _batches_cpu(self) -> Iterator[Tuple[torch.Tensor, torch.Tensor]]:
        pool = ThreadPoolExecutor(max_workers=self.workers)
        try:
            rows = self._iter_rows()
            while True:
                chunk = []
                for _ in range(self.batch_size):
                    try:
                        chunk.append(next(rows))
                    except StopIteration:
                        break
                if not chunk:
                    return
                futs = [pool.submit(self.transform, c) for c, _ in chunk]
                images = torch.stack([f.result() for f in futs])
                labels = torch.tensor([l for _, l in chunk], dtype=torch.long)
                yield images, labels
                if len(chunk) < self.batch_size:
                    return
        finally:
            pool.shutdown(wait=False)

    def _batches_proc(self, owner: Optional[dict] = None) -> Iterator[Tuple[torch.Tensor, torch.Tensor, Callable]]:
        """Decode batches via the process pool. Yields
        ``(images_view, labels, release)`` where ``images_view`` is a
        zero-copy torch view over a shared-memory slot: the consumer must
        copy it out (to pinned / to an owned tensor) and then call
        ``release()`` to return the slot to the ring. Batch order is
        deterministic (seq-reordered) regardless of worker scheduling."""
        rows = self._iter_rows()
        first = next(rows, None)
        if first is None:
            return
        sample = self.transform(first[0])
        if isinstance(sample, torch.Tensor):
            sample = sample.numpy()
        sample = np.asarray(sample)
        rows = itertools.chain([first], rows)

        pool = _ProcDecodePool(
            self.transform, sample.shape, sample.dtype, self.batch_size,
            self.workers,
            pin=self.device is not None and self.device.type == "cuda")
        if owner is not None:
            # the consumer owns teardown: the pinned shm ring must outlive
            # its in-flight H2D DMA, which only the consumer can order
            # (generator exhaustion happens BEFORE the last stage is issued)
            owner["pool"] = pool
        self._pool_info = (pool.slots, pool.pinned)
        free_slots: deque = deque(range(pool.slots))
        pending_labels = {}
        heap: list = []
        submit_seq = 0
        yield_seq = 0
        exhausted = False
        try:
            while True:
                while free_slots and not exhausted:
                    chunk = list(itertools.islice(rows, self.batch_size))
                    if not chunk:
                        exhausted = True
                        break
                    slot = free_slots.popleft()
                    pool.task_q.put((submit_seq, slot, [c for c, _ in chunk]))
                    pending_labels[submit_seq] = torch.tensor(
                        [l for _, l in chunk], dtype=torch.long)
                    submit_seq += 1
                    if len(chunk) < self.batch_size:
                        exhausted = True
                if exhausted and yield_seq == submit_seq:
                    return
                stall = 0.0
                while not heap or heap[0][0] != yield_seq:
                    try:
                        status, seq, slot, payload = pool.res_q.get(timeout=5.0)
                    except queue.Empty:
                        dead = pool.any_dead()
                        if dead:
                            raise RuntimeError(
                                f"decode worker(s) died (pids {dead})")
                        stall += 5.0
                        if stall >= 120.0:
                            # alive-but-wedged workers (fork-after-CUDA
                            # hazard): fail loudly instead of hanging
                            raise RuntimeError(
                                "decode pool made no progress for 120s "
                                "(workers alive but wedged)")
                        continue
                    stall = 0.0
                    if status == "err":
                        raise RuntimeError(f"decode failed in worker: {payload}")
                    heapq.heappush(heap, (seq, slot, payload))
                seq, slot, n = heapq.heappop(heap)
                labels = pending_labels.pop(seq)
                imgs = torch.from_numpy(pool.view[slot, :n])
                # deque.append is atomic -> safe to call from a consumer thread
                yield imgs, labels, (lambda s=slot: free_slots.append(s))
                yield_seq += 1
        finally:
            if owner is None:
                pool.close()

    def _resolve_pool(self) -> str:
        if self.pool != "auto":
            return self.pool
        import multiprocessing as mp

        if mp.current_process().daemon:
            return "thread"  # daemonic processes cannot fork children
        # processes pay off where decode must keep up with a GPU; the CPU
        # path keeps the cheap thread pool (tests, small oracle runs)
        return "process" if (self.device is not None and self.device.type != "cpu") else "thread"

    def __iter__(self):
        mode = self._resolve_pool()
        if self.device is None or self.device.type == "cpu":
            if mode == "process":
                for imgs, labels, release in self._batches_proc():
                    out = imgs.clone()
                    release()
                    yield out, labels
            else:
                yield from self._batches_cpu()
            return
        # GPU path: background decode (process pool or thread pool) + pinned
        # double-buffer staging on a side stream
        if self._stager is None:
            self._stager = _H2DStager(self.device, depth=max(2, self.prefetch))
        q: "queue.Queue" = queue.Queue(maxsize=self.prefetch)
        stop = threading.Event()

        def _bounded_put(item) -> bool:
            # bounded put so the thread can exit promptly once the
            # consumer is gone (avoids a blocked thread at teardown)
            while not stop.is_set():
                try:
                    q.put(item, timeout=0.25)
                    return True
                except queue.Full:
                    continue
            return False

        pool_owner: dict = {}

        def producer():
            try:
                if mode == "process":
                    for imgs, labels, release in self._batches_proc(pool_owner):
                        if not _bounded_put((imgs, labels, release)):
                            release()
                            return
                else:
                    for batch in self._batches_cpu():
                        if not _bounded_put((batch[0], batch[1], None)):
                            return
            finally:
                # the end-of-stream sentinel must ARRIVE: a put_nowait here
                # is silently dropped when the bounded queue is full (fast
                # decode pool, consumer still staging) and the consumer
                # then blocks on q.get() forever — the late-session GPU
                # hang. Bounded-put it like any other item.
                _bounded_put(None)

        t = threading.Thread(target=producer, daemon=True)
        t.start()
        pending: deque = deque()  # (event, release): slots with H2D in flight
        try:
            while True:
                item = q.get()
                if item is None:
                    return
                imgs, labels, release = item
                pool_slots, pool_pinned = getattr(self, "_pool_info", (0, False))
                if release is not None and pool_pinned:
                    # slot ring is hipHostRegister-ed: DMA straight from the
                    # slot on the side stream; the slot is released once the
                    # copy's event completes (deferred, non-blocking drain)
                    ev = torch.cuda.Event()
                    with torch.cuda.stream(self._stager.stream):
                        di = imgs.to(self.device, non_blocking=True)
                        dl = labels.to(self.device, non_blocking=True)
                        ev.record(self._stager.stream)
                    pending.append((ev, release))
                    while pending and pending[0][0].query():
                        pending.popleft()[1]()
                    if len(pending) >= max(2, pool_slots - 2):
                        ev0, rel0 = pending.popleft()
                        ev0.synchronize()
                        rel0()
                else:
                    di, dl, ev = self._stager.stage(imgs, labels)
                    if release is not None:
                        release()  # stage() memcpy'd the slot into pinned
                cs = torch.cuda.current_stream(self.device)
                cs.wait_event(ev)
                # the device tensors were allocated on the side stream; tell
                # the caching allocator they are consumed on the compute
                # stream, or a freed block could be handed to a later
                # side-stream H2D copy while compute still reads it
                di.record_stream(cs)
                dl.record_stream(cs)
                yield di, dl
        finally:
            # order matters: finish in-flight DMA from the pinned shm ring
            # BEFORE the pool (hostUnregister + unmap) can tear down — the
            # consumer owns the pool exactly for this reason
            if pending:
                torch.cuda.synchronize(self.device)
                while pending:
                    pending.popleft()[1]()
            stop.set()
            # drain so the producer can exit, then join it so no thread is
            # left inside native code at interpreter teardown
            while not q.empty():
                try:
                    item = q.get_nowait()
                    if item is not None and item[2] is not None:
                        item[2]()
                except queue.Empty:
                    break
            t.join(timeout=10.0)
            pool = pool_owner.get("pool")
            if pool is not None:
                if pool.pinned:
                    torch.cuda.synchronize(self.device)
                pool.close()


class Converter:
    """Petastorm ``SparkDatasetConverter`` equivalent over a cached Parquet
    dataset (``make_spark_converter`` contract)."""

    def __init__(self, cache_path: Path, owned: bool):
        self.path = Path(cache_path)
        self._owned = owned
        self._len = sum(
            pq.ParquetFile(f).metadata.num_rows for f in sorted(self.path.glob("*.parquet"))
        )

    def __len__(self) -> int:
        return self._len

    class _DatasetCtx:
        def __init__(self, loader: "ShardedParquetLoader"):
            self.loader = loader

        def __enter__(self) -> "ShardedParquetLoader":
            return self.loader

        def __exit__(self, *exc) -> None:
            pass

    def make_torch_dataset(
        self,
        batch_size: int = 32,
        cur_shard: int = 0,
        shard_count: int = 1,
        num_epochs: Optional[int] = None,
        workers_count: int = 4,
        device: Optional[torch.device] = None,
        **kw,
    ) -> "Converter._DatasetCtx":
        loader = ShardedParquetLoader(
            str(self.path),
            batch_size=batch_size,
            cur_shard=cur_shard,
            shard_count=shard_count,
            num_epochs=num_epochs,
            workers=workers_count,
            device=device,
            **kw,
        )
        return Converter._DatasetCtx(loader)

    def delete(self) -> None:
        import shutil

        if self._owned and self.path.exists():
            shutil.rmtree(self.path)


def make_converter(
    source,
    cache_dir: Optional[str] = None,
    row_group_rows: int = 64,
) -> Converter:
    """Build a converter from a pyarrow Table (materialised to a Parquet cache
    dir, like ``make_spark_converter``) or an existing Parquet dataset path."""
    if isinstance(source, (str, Path)):
        return Converter(Path(source), owned=False)
    if not isinstance(source, pa.Table):
        raise TypeError(f"unsupported source {type(source)}")
    cache_root = Path(cache_dir or (Path(current_setup().root) / "cache"))
    dst = cache_root / f"converter-{uuid.uuid4().hex[:12]}"
    dst.mkdir(parents=True, exist_ok=True)
    pq.write_table(source, dst / "part-00000.parquet", row_group_size=row_group_rows, compression="NONE")
    return Converter(dst, owned=True)
