"""What the sync round's options, the timestamp classifier and the export cost
("Async rounds and a hand-over that keeps state").

  python tools/sync_options_measure.py ROOT MODE...

runs config 3's device-resident round (the bodies of tools/e2e_host.py:
100,000 all-canonical SyncRequest bodies, E2E_OWNERS to shrink) from the built
tree at ROOT: one warm round, then three timed rounds per MODE, the modes
alternating, each round on a fresh server.  MODEs:
  none    no evm_sync_set_option call (the only mode a tree from before the
          options knows: ROOT = a built checkout of that commit)
  off     both options set to 0
  on      both options set to 1
  extras  also k_ts_classify's time at 1M rows (evm_prof_report; canonical
          rows, and tests/golden/js_lenient.json tiled) and evm_sync_export's
          wall time for one 1,000-row user and for 1,000 users in one call
To compare two commits run the two trees in separate processes, alternating
(A, B, A, B): two processes of one build differ by 0.3-0.5 ms.
The last line is "RESULT " + JSON."""
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.abspath(sys.argv[1])
MODES = sys.argv[2:]
sys.path.insert(0, ROOT)
os.chdir(ROOT)
import bench  # noqa: E402
from evolu_amd import synth  # noqa: E402
from evolu_amd.engine import Engine  # noqa: E402
from evolu_amd.server import SyncServer  # noqa: E402

owners, per = int(os.environ.get("E2E_OWNERS", 100_000)), 1000
out = {"root": ROOT, "owners": owners}
t0 = time.perf_counter()
ts_np, owner_np, millis = synth.config3(owners, per, seed_config=3, request=per)
eng = Engine(0)
dev = torch.device("cuda", 0)
ts_r = eng.dev(ts_np)
lown = torch.from_numpy(owner_np.astype(np.int32)).to(dev)
o64 = owner_np.astype(np.int64)
order = np.lexsort((millis, o64))
rank = np.empty(len(order), dtype=np.int64)
cnt = np.bincount(o64, minlength=owners)
rank[order] = np.arange(len(order)) - (np.cumsum(cnt) - cnt)[o64[order]]
keep = torch.from_numpy(rank < (0.9 * cnt[o64]).astype(np.int64)).to(dev)
client = eng.merkle_insert(eng.tree_new(owners), ts_r[keep].contiguous(), lown[keep].contiguous())
arena, off = bench.e2e_bodies(eng, ts_np, owner_np, client)
del lown, keep
client.free()
print("bodies ready: %d bytes in %.0f s" % (int(off[-1]), time.perf_counter() - t0), flush=True)
a_d = torch.from_numpy(arena).to(dev)


def server(mode):
    srv = SyncServer(eng, owners)
    if mode != "none":
        v = 1 if mode == "on" else 0
        for opt in (1, 2):
            assert eng.lib.evm_sync_set_option(srv.h, opt, v) == 0
    return srv


def one_round(mode):
    srv = server(mode)
    torch.cuda.synchronize()
    t = time.perf_counter()
    res = srv.sync_device(a_d, off)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t) * 1e3
    parts = {k: round(v * 1e3, 2) for k, v in srv.timing.items()}
    del res
    return srv, ms, parts


srv, ms, _ = one_round(MODES[0] if MODES[0] != "extras" else "none")  # warm
srv.close()
print("warm round %.1f ms" % ms, flush=True)
for rep in range(3):  # (the modes alternate: a drift of the machine shows in both)
    for mode in [m for m in MODES if m != "extras"]:
        srv, ms, parts = one_round(mode)
        srv.close()
        out.setdefault(mode, []).append(round(ms, 2))
        print("mode %s round %.2f ms" % (mode, ms), parts, flush=True)

if "extras" in MODES:
    lib = eng.lib
    # ---- classifier: 1M canonical rows, 1M rows of the V8 vectors tiled
    vec = json.load(open(os.path.join(ROOT, "tests", "golden", "js_lenient.json")))["vectors"]
    v = np.zeros((len(vec), 48), dtype=np.uint8)
    v[:, :46] = np.frombuffer("".join(x["raw"] for x in vec).encode(), dtype=np.uint8).reshape(len(vec), 46)
    n = 1_000_000
    sets = {"canonical": ts_r[:n].contiguous(), "v8_vectors_tiled": eng.dev(np.tile(v, (n // len(vec) + 1, 1))[:n])}
    for name, rows in sets.items():
        eng.classify_timestamps(rows)  # warm
        eng.prof_enable(True)
        eng.prof_reset()
        for _ in range(5):
            cls, canon = eng.classify_timestamps(rows)
        rep = eng.prof_report()
        eng.prof_enable(False)
        tot, launches = rep["k_ts_classify"]
        out["classify_" + name] = {"rows": n, "ms_per_call": tot / launches, "ns_per_row": tot / launches * 1e6 / n,
                                   "classes": np.bincount(cls.cpu().numpy(), minlength=3).tolist()}
        print("classify", name, out["classify_" + name], flush=True)
    del ts_r
    # ---- export: one 1,000-row user; 1,000 users in one call (a server holding the round's rows)
    from tests.test_wire import RESP

    srv, ms, _ = one_round("on")

    def export(slots):
        sl = np.asarray(slots, dtype=np.uint32)
        roff, total = np.zeros(len(sl) + 1, dtype=np.uint64), C.c_uint64()
        torch.cuda.synchronize()
        t = time.perf_counter()
        st = lib.evm_sync_export(srv.h, sl.ctypes.data_as(C.c_void_p), len(sl), roff.ctypes.data_as(C.c_void_p),
                                 C.byref(total))
        dt = time.perf_counter() - t
        assert st == 0, st
        return dt, roff, total.value

    for name, slots in (("one_user", [owners // 2]), ("thousand_users", list(range(7, 7 + 1000)))):
        export(slots)  # warm
        times = []
        for _ in range(3):
            dt, roff, total = export(slots)
            times.append(dt)
        buf = np.zeros(total, dtype=np.uint8)
        assert lib.evm_sync_fetch(srv.h, buf.ctypes.data_as(C.c_void_p)) == 0
        rows = sum(len(RESP.FromString(buf[int(roff[k]):int(roff[k + 1])].tobytes()).messages)
                   for k in range(len(slots)))
        out["export_" + name] = {"rows": rows, "bytes": int(total), "ms": [round(t * 1e3, 3) for t in times],
                                 "rows_per_s": rows / min(times)}
        print("export", name, out["export_" + name], flush=True)
    srv.close()
print("RESULT " + json.dumps(out), flush=True)
