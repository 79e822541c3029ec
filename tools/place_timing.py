"""Place recognition: visfs_place_query of 500 key-points against 30 (Mem/STMSize), 256 and 1024 key-frames of 500 entries
(Kp/MaxFeatures), and visfs_place_describe of 500 key-points on a resident 752 x 480 image, on the GPU and on the host twin (one core)
of the same machine.  Median of --calls calls after --warmup warm-ups of the same shapes.  A query ends in its own device
synchronise; a describe does not wait, so it is timed together with a download of its valid flags, which does.  Descriptors are
random bits with near copies of the queries planted in one slot, so the accept rule has work to do.  Prints a table and one JSON
line (and --out FILE).

    python tools/place_timing.py [--calls 500] [--host-calls 3] [--warmup 20] [--out profiles/place_timing.log]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from visfs_amd import abi, backend  # noqa: E402
from visfs_amd import flow, place  # noqa: E402
import flow_cases as fc  # noqa: E402

N = 500


def stats(t):
    return float(np.median(t)) * 1e3, float(np.min(t)) * 1e3, float(np.max(t)) * 1e3, float(np.sum(t))


def time_query(db, dset, calls, warmup):
    lib = place.load()
    p, r = place.default_params(), place.Result()
    t = []
    for i in range(calls + warmup):
        t0 = time.perf_counter()
        rc = lib.visfs_place_query(db.h, dset.h, C.byref(p), C.byref(r))
        t1 = time.perf_counter()
        assert rc == abi.OK, db.last_error()
        if i >= warmup:
            t.append(t1 - t0)
    return stats(t), bytes(memoryview(r))


def time_describe(dset, xy, calls, warmup):
    lib = place.load()
    valid = np.zeros(len(xy), dtype=np.uint8)
    n = C.c_int32(0)
    pf, pu8 = C.POINTER(C.c_float), C.POINTER(C.c_uint8)
    t = []
    for i in range(calls + warmup):
        t0 = time.perf_counter()
        rc = lib.visfs_place_describe(dset.h, place.SLOT_CURRENT, place.IMAGE_LEFT, len(xy), xy.ctypes.data_as(pf))
        rc2 = lib.visfs_place_set_download(dset.h, C.byref(n), None, None, valid.ctypes.data_as(pu8), None)
        t1 = time.perf_counter()
        assert rc == abi.OK and rc2 == abi.OK, dset.last_error()
        if i >= warmup:
            t.append(t1 - t0)
    return stats(t), dset.download()["desc"].tobytes()


def fill(stores, sets, n_slots, rng, q):
    for k in range(n_slots):
        d = rng.integers(0, 256, (N, 32), dtype=np.uint8)
        if k == n_slots // 2:                                  # the revisited place: 300 of the queries, 8 bits flipped
            d[:300] = q[100:400]
            for row in d[:300]:
                for b in rng.choice(256, 8, replace=False):
                    row[b >> 3] ^= np.uint8(1 << (b & 7))
        ids, xyz = np.arange(N, dtype=np.int32), rng.normal(0, 3, (N, 3)).astype(np.float32)
        for s, db in zip(sets, stores):
            s.upload(np.zeros((N, 2), np.float32), d, np.ones(N, np.uint8))
            db.add(s, ids, xyz, k)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=500)
    ap.add_argument("--host-calls", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    w, h = 752, 480
    img = fc.base_image(w, h)
    s = backend.Solver(abi.default_params())                  # raises without a GPU: there is no number to report then
    dev, host = flow.Flow(flow.default_params(), w, h, solver=s), flow.Flow(flow.default_params(), w, h)
    dev.push_frame(img, img)
    host.push_frame(img, img)
    sets = [place.DescriptorSet(dev, 512), place.DescriptorSet(host, 512)]
    lines = [f"place_timing: {N} key-points; median (min .. max) ms of {a.calls} GPU calls / {a.host_calls} host-twin calls after warm-ups of the "
             f"same shapes; host twin: one core of the same machine",
             f"{'case':<40}{'GPU':>30}{'host twin':>34}  identical"]
    record = {}
    rng = np.random.default_rng(5)
    xy = np.stack([rng.uniform(10, w - 11, N), rng.uniform(10, h - 11, N)], -1).astype(np.float32)
    g, gd = time_describe(sets[0], xy, a.calls, a.warmup)
    c, cd = time_describe(sets[1], xy, max(a.host_calls, 5), 1)
    lines.append(f"{'describe 500 on 752 x 480 + download':<40}{g[0]:>10.4f} ({g[1]:.4f} .. {g[2]:.4f}){c[0]:>14.3f} ({c[1]:.3f} .. {c[2]:.3f})  {gd == cd}")
    record["describe"] = dict(gpu_ms_median=g[0], host_1core_ms_median=c[0], identical=gd == cd, gpu_timed_s=g[3])
    for n_slots in (30, 256, 1024):
        stores = [place.KeyFrameStore(s, n_slots), place.KeyFrameStore(None, n_slots)]
        q = rng.integers(0, 256, (N, 32), dtype=np.uint8)
        fill(stores, sets, n_slots, rng, q)
        for st in sets:
            st.upload(xy, q, np.ones(N, np.uint8))
        g, gr = time_query(stores[0], sets[0], a.calls, a.warmup)
        c, cr = time_query(stores[1], sets[1], a.host_calls, 1)
        got = place.unpack(np.frombuffer(gr, dtype=np.uint8).ctypes.data_as(C.POINTER(place.Result)).contents)
        top = got["candidates"][0] if got["candidates"] else dict(slot=-1, count=0)
        pairs = n_slots * N * N
        name = f"query, {n_slots} slots of {N}"
        lines.append(f"{name:<40}{g[0]:>10.4f} ({g[1]:.4f} .. {g[2]:.4f}){c[0]:>14.3f} ({c[1]:.3f} .. {c[2]:.3f})  {gr == cr}")
        lines.append(f"{'':<40}  top slot {top['slot']} with {top['count']} rows; {pairs:.3g} descriptor pairs, each met twice (rows, then columns): "
                     f"{2 * pairs / (g[0] * 1e-3):.3g} distances/s; timed window: GPU {g[3]:.3f} s, host twin {c[3]:.3f} s")
        record[name] = dict(gpu_ms_median=g[0], host_1core_ms_median=c[0], identical=gr == cr, top_slot=top["slot"], top_count=top["count"],
                            gpu_timed_s=g[3])
        for st in stores:
            st.close()
    lines.append(json.dumps(dict(tool="place_timing", points=N, calls=a.calls, warmup=a.warmup, cases=record)))
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")
    for st in sets:
        st.close()
    dev.close(); host.close(); s.close()


if __name__ == "__main__":
    main()
