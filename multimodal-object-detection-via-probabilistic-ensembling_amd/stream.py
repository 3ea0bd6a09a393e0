"""Streaming, rank-sharded FLIR frame-pair loader (the host side of `demo_probEn --one-pass`).

The reference decodes one frame pair at a time in the driver's process and builds the fusion inputs on the host
(demo/FLIR/demo_FLIR_save_predictions.py:98-121).  Here JPEG decode - the only host work left, data.read_image = PIL - runs in
worker processes; everything after it happens on the GPU (pe_fusion_input_pack).

    loader = FlirPairLoader(dataset_path, batch=32, need_rgb=True, workers=4)
    for b in loader:        # this rank's comm.shard_range block, in dataset order
        b.ids, b.names, b.hw, b.thermal, b.rgb      # pinned uint8 [B,H,W,3] BGR batches (rgb None unless need_rgb)

Workers (spawn context) never open the GPU: they decode into shared-memory slots, one frame pair per slot, and the main
process copies the slots into page-locked batch buffers in dataset order.  Only slot numbers and shapes are pickled (a frame
larger than its slot travels pickled once and the slot grows).  At most `prefetch` pairs are decoded ahead.  A frame pair
whose sizes differ from the current batch's closes that batch.  `workers=0` decodes in-process.

A yielded batch's host tensors are reused two batches later: finish reading them (e.g. the H2D copy) before asking for the
batch after next."""
import json
import multiprocessing as mp
import os
import queue
import time
from multiprocessing import shared_memory

import numpy as np

from . import comm
from .data import read_image

DEFAULT_WORKERS = 4    # the reference's DATALOADER.NUM_WORKERS
MAX_WORKERS = 15       # leaves one of a 16-CPU share for the driver


def flir_pairs(dataset_path):
    """FLIR val layout: FLIR_thermal_RGBT_pairs_val.json, thermal_8_bit/<stem>.jpeg, RGB/<stem>.jpg.  One dict per pair in
    json order: id, name (<stem>.jpeg, the J1 `image` entry), thermal / rgb paths, thermal (height, width)."""
    with open(os.path.join(dataset_path, "FLIR_thermal_RGBT_pairs_val.json")) as f:
        images = json.load(f)["images"]
    out = []
    for im in images:
        stem = os.path.splitext(os.path.basename(im["file_name"]))[0]
        out.append({"id": im["id"], "name": stem + ".jpeg", "hw": (im["height"], im["width"]),
                    "thermal": os.path.join(dataset_path, "thermal_8_bit", stem + ".jpeg"),
                    "rgb": os.path.join(dataset_path, "RGB", stem + ".jpg")})
    return out


def check_workers(workers):
    workers = DEFAULT_WORKERS if workers is None else int(workers)
    if not 0 <= workers <= MAX_WORKERS:
        raise ValueError(f"--workers {workers}: 0 (decode in-process) .. {MAX_WORKERS}")
    return workers


def decode_pair(item, need_rgb):
    t = read_image(item["thermal"], "BGR")
    return t, (read_image(item["rgb"], "BGR") if need_rgb else None)


def _worker(tasks, results):
    """Decode loop of one worker process.  Touches no GPU API: only PIL, numpy and shared memory."""
    slots = {}
    while True:
        task = tasks.get()
        if task is None:
            break
        if task[0] == "probe":
            import sys
            torch = sys.modules.get("torch")
            results.put(("probe", os.getpid(), bool(torch is not None and torch.cuda.is_initialized())))
            break                   # one answer per worker
        _, i, slot, name, cap, item, need_rgb = task
        try:
            frames = [f for f in decode_pair(item, need_rgb) if f is not None]
            shapes = [f.shape for f in frames]
            if sum(f.nbytes for f in frames) > cap:
                results.put((i, slot, shapes, b"".join(f.tobytes() for f in frames), None))
                continue
            if name not in slots:
                slots[name] = shared_memory.SharedMemory(name=name)
            off = 0
            for f in frames:
                np.ndarray(f.shape, np.uint8, buffer=slots[name].buf, offset=off)[...] = f
                off += f.nbytes
            results.put((i, slot, shapes, None, None))
        except Exception as e:   # noqa: BLE001 - reported in the main process with the file names
            results.put((i, slot, None, None, f"{type(e).__name__}: {e}"))
    for s in slots.values():
        s.close()


class PairBatch:
    def __init__(self, ids, names, hw, thermal, rgb):
        self.ids, self.names, self.hw, self.thermal, self.rgb = ids, names, hw, thermal, rgb

    def __len__(self):
        return len(self.ids)


class FlirPairLoader:
    def __init__(self, dataset_path, batch, need_rgb=True, workers=None, prefetch=None, pin=None, rank=None, world=None):
        import torch
        self.items = flir_pairs(dataset_path)
        self.mine = comm.shard_range(len(self.items), rank, world)
        self.batch = int(batch)
        assert self.batch >= 1
        self.need_rgb = bool(need_rgb)
        self.workers = check_workers(workers)
        self.prefetch = int(prefetch) if prefetch else max(2 * self.batch, 4 * self.workers)
        self.pin = torch.cuda.is_available() if pin is None else bool(pin)
        self.wait_s = 0.0          # time the consumer spent blocked on decode (workers: waiting for a slot; 0 workers: decoding)
        self._bufs = {}            # batch shape -> two host buffer sets, used alternately
        self._flip = 0

    def __len__(self):
        return len(self.mine)

    # ------------------------------------------------------------------ frames in dataset order
    def _frames_inline(self):
        for i in self.mine:
            t0 = time.perf_counter()
            t, r = decode_pair(self.items[i], self.need_rgb)
            self.wait_s += time.perf_counter() - t0
            yield i, t, r

    def _frames_workers(self):
        ctx = mp.get_context("spawn")
        tasks, results = ctx.Queue(), ctx.Queue()
        procs = [ctx.Process(target=_worker, args=(tasks, results), daemon=True) for _ in range(self.workers)]
        for p in procs:
            p.start()
        first = self.items[self.mine[0]]
        from PIL import Image
        cap = 3 * first["hw"][0] * first["hw"][1]
        if self.need_rgb:
            with Image.open(first["rgb"]) as im:      # header only: sizes the slots for the RGB frames too
                cap += 3 * im.size[0] * im.size[1]
        nslot = min(self.prefetch, len(self.mine))
        shms = [shared_memory.SharedMemory(create=True, size=cap) for _ in range(nslot)]
        order = list(self.mine)
        nxt = 0
        frames = buf = None

        def issue(slot):
            nonlocal nxt
            if nxt < len(order):
                s = shms[slot]
                tasks.put(("decode", order[nxt], slot, s.name, s.size, self.items[order[nxt]], self.need_rgb))
                nxt += 1
        try:
            for s in range(nslot):
                issue(s)
            done = {}
            for i in order:
                t0 = time.perf_counter()
                while i not in done:
                    try:
                        r = results.get(timeout=5.0)
                    except queue.Empty:
                        dead = [p.exitcode for p in procs if not p.is_alive()]
                        if dead:
                            raise RuntimeError(f"FlirPairLoader: a decode worker exited (codes {dead})") from None
                        continue
                    done[r[0]] = r
                self.wait_s += time.perf_counter() - t0
                _, slot, shapes, payload, err = done.pop(i)
                if err is not None:
                    it = self.items[i]
                    raise RuntimeError(f"FlirPairLoader: decoding {it['thermal']} / {it['rgb']} failed: {err}")
                if payload is not None:
                    buf = memoryview(payload)
                    need = len(payload)
                    shms[slot].close()
                    shms[slot].unlink()
                    shms[slot] = shared_memory.SharedMemory(create=True, size=need)     # the next frames of this size fit
                else:
                    buf = shms[slot].buf
                frames, off = [], 0
                for shp in shapes:
                    n = int(np.prod(shp))
                    frames.append(np.ndarray(shp, np.uint8, buffer=buf, offset=off))
                    off += n
                yield i, frames[0], (frames[1] if self.need_rgb else None)
                del frames, buf      # the consumer has copied the pair out: the slot is free again
                issue(slot)
        finally:
            frames = buf = None
            for _ in procs:
                tasks.put(None)
            for p in procs:
                p.join(timeout=10)
                if p.is_alive():
                    p.terminate()
            for s in shms:
                try:
                    s.close()
                except BufferError:      # a consumer that stopped early still holds a view: the mapping goes with the process
                    pass
                s.unlink()

    def frames(self):
        """(dataset index, thermal uint8 [H,W,3], rgb uint8 [H,W,3] | None) in dataset order; the arrays are only valid until
        the next item is requested."""
        if len(self.mine) == 0:
            return iter(())
        return self._frames_workers() if self.workers > 0 else self._frames_inline()

    # ------------------------------------------------------------------ batches
    def _host(self, shape_key):
        if shape_key not in self._bufs:
            self._bufs = {}           # one live shape at a time: a size change is a batch boundary
            self._bufs[shape_key] = [[self._alloc((self.batch,) + tuple(s)) for s in shape_key] for _ in range(2)]
        k = self._flip
        self._flip ^= 1
        return self._bufs[shape_key][k]

    def _alloc(self, shape):
        import torch
        t = torch.empty(shape, dtype=torch.uint8)
        return t.pin_memory() if self.pin else t

    def __iter__(self):
        host, key, idx = None, None, []

        def close():
            n = len(idx)
            return PairBatch([self.items[i]["id"] for i in idx], [self.items[i]["name"] for i in idx], key[0][:2],
                             host[0][:n], host[1][:n] if self.need_rgb else None)
        for i, t, r in self.frames():
            fr = [t] + ([r] if r is not None else [])
            k = tuple(f.shape for f in fr)
            if host is not None and (len(idx) == self.batch or k != key):
                yield close()
                host = None
            if host is None:
                host, key, idx = self._host(k), k, []
            for h, f in zip(host, fr):
                h[len(idx)].numpy()[...] = f
            idx.append(i)
        if host is not None:
            yield close()

    def probe_workers(self):
        """Start the workers, ask each whether torch.cuda is initialised in it (each answers once and exits; tests)."""
        ctx = mp.get_context("spawn")
        tasks, results = ctx.Queue(), ctx.Queue()
        procs = [ctx.Process(target=_worker, args=(tasks, results), daemon=True) for _ in range(self.workers)]
        for p in procs:
            p.start()
        try:
            for _ in procs:
                tasks.put(("probe",))
            return [results.get(timeout=120)[1:] for _ in procs]
        finally:
            for p in procs:
                p.join(timeout=10)
