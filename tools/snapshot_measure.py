"""Measures SyncServer.compact / save / load ("Restart").

    python tools/snapshot_measure.py --owners 100000 --per-owner 1000 --dir /tmp --out bench_out/snapshot.json

The history is the config-3 end-to-end round (bench.e2e_bodies: one
SyncRequest of --per-owner messages per owner, 16-B contents, the client
knowing each owner's oldest 90 %), then a resend round: the first
--resend of the bodies again, every row of it dead.  Measured:

  compaction   HIP-event time on the engine's stream, the bytes it has to move
               (ids read and written once, live rows, offsets and contents
               read once and written once), the share of 8 TB/s, and a plain
               device-to-device copy of the same bytes in the same run
  save, load   wall time and file bytes per second (the staged D2H / H2D rates
               of host rounds are 51 and 56.6 GB/s), and the file system
  replay       the alternative a server without snapshots has: the same
               bodies through sync_arena on a fresh server
  memory       log bytes, free device memory and the per-round segment
               descriptors before and after compacting ~50 small rounds

One JSON object per line on stdout (and in --out)."""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

HBM_BYTES_PER_S = 8e12
_STREAMS = []  # (the engine keeps using a bound stream: it must outlive the call that made it)
SEG_DESCRIPTOR_BYTES = 40  # per segment and round: base, row map, ts, offsets, contents (8 B each)


def emit(out, rec):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


def history(eng, owners, per_owner, resend):
    """(arena, off) of the first round, (arena, off) of the resend round."""
    import bench
    from evolu_amd import synth

    ts_np, owner_np, millis = synth.config3(owners, per_owner, seed_config=3, request=per_owner)
    o64 = owner_np.astype(np.int64)
    order = np.lexsort((millis, o64))
    rank = np.empty(len(order), dtype=np.int64)
    cnt = np.bincount(o64, minlength=owners)
    rank[order] = np.arange(len(order)) - (np.cumsum(cnt) - cnt)[o64[order]]
    keep = rank < (0.9 * cnt[o64]).astype(np.int64)
    client = eng.merkle_insert(eng.tree_new(owners), eng.dev(np.ascontiguousarray(ts_np[keep])),
                               eng.dev(np.ascontiguousarray(owner_np[keep])))
    arena, off = bench.e2e_bodies(eng, ts_np, owner_np, client)
    client.free()
    k = int(round(resend * (len(off) - 1)))
    return (arena, off), (arena[: int(off[k])], np.ascontiguousarray(off[: k + 1]))


def log_bytes(info):
    return info["rows"] * 56 + 8 * info["segments"] + info["content_bytes"]


def d2d_copy_ms(nbytes, reps=5):
    """A device-to-device copy that reads nbytes / 2 and writes nbytes / 2."""
    a = torch.empty(nbytes // 2, dtype=torch.uint8, device="cuda")
    b = torch.empty_like(a)
    a.zero_()
    b.copy_(a)
    torch.cuda.synchronize()
    best = None
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        b.copy_(a)
        e1.record()
        e1.synchronize()
        ms = e0.elapsed_time(e1)
        best = ms if best is None else min(best, ms)
    del a, b
    torch.cuda.empty_cache()
    return best


def measure(eng, a, owners, per_owner, out):
    from evolu_amd.server import SyncServer, snapshot_info

    name = "%d owners x %d" % (owners, per_owner)
    t0 = time.perf_counter()
    (arena, off), (arena2, off2) = history(eng, owners, per_owner, a.resend)
    emit(out, {"step": "history", "size": name, "s": time.perf_counter() - t0, "request_bytes": int(off[-1]),
               "resend_bytes": int(off2[-1])})
    srv = SyncServer(eng, owners)
    srv.sync_arena(arena, off)
    srv.sync_arena(arena2, off2)
    before = srv.log_info()
    n = srv.store.n_messages
    free0, _ = torch.cuda.mem_get_info()
    # ---- compaction, timed by HIP events on the engine's stream
    stream = torch.cuda.Stream()
    _STREAMS.append(stream)
    eng.bind_stream(stream)
    eng.prof_reset()
    eng.prof_enable(True)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    t0 = time.perf_counter()
    srv.compact()
    wall = time.perf_counter() - t0
    e1.record(stream)
    e1.synchronize()
    ms = e0.elapsed_time(e1)
    prof = eng.prof_report()
    eng.prof_enable(False)
    after = srv.log_info()
    free1, _ = torch.cuda.mem_get_info()
    moved = 128 * n + 2 * after["content_bytes"]
    copy_ms = d2d_copy_ms(moved)
    emit(out, {"step": "compact", "size": name, "rows_before": before["rows"], "rows_after": after["rows"],
               "dead_share": 1 - after["rows"] / before["rows"], "segments_before": before["segments"],
               "event_ms": ms, "wall_ms": wall * 1e3, "bytes_moved": moved, "gb_per_s": moved / ms / 1e6,
               "share_of_8_tb_per_s": moved / (ms / 1e3) / HBM_BYTES_PER_S, "d2d_copy_ms": copy_ms,
               "d2d_copy_gb_per_s": moved / copy_ms / 1e6, "ratio_to_d2d_copy": ms / copy_ms,
               "log_bytes_before": log_bytes(before), "log_bytes_after": log_bytes(after),
               "device_free_gained": int(free1 - free0),
               "kernels_ms": {k: round(v[0], 3) for k, v in sorted(prof.items(), key=lambda kv: -kv[1][0])[:8]}})
    # ---- save, load, replay
    path = os.path.join(a.dir, "evm_snapshot_measure_%d.snap" % os.getpid())
    t0 = time.perf_counter()
    srv.save(path)
    save_s = time.perf_counter() - t0
    size = os.path.getsize(path)
    t0 = time.perf_counter()
    srv.save(path)
    save2_s = time.perf_counter() - t0
    roots = srv.store.tree().roots()
    next_id = srv.next_id
    srv.close()
    t0 = time.perf_counter()
    info = snapshot_info(path)
    verify_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    back = SyncServer.load(eng, path, owners)
    load_s = time.perf_counter() - t0
    r2 = back.store.tree().roots()
    same = bool(back.next_id == next_id and back.store.n_messages == n and (r2[0] == roots[0]).all()
                and (r2[1] == roots[1]).all())
    back.close()
    fresh = SyncServer(eng, owners)
    t0 = time.perf_counter()
    fresh.sync_arena(arena, off)
    replay1_s = time.perf_counter() - t0
    fresh.sync_arena(arena2, off2)
    replay_s = time.perf_counter() - t0
    r3 = fresh.store.tree().roots()
    same = same and bool((r3[0] == roots[0]).all())
    fresh.close()
    df = subprocess.run(["df", "-PT", a.dir], capture_output=True, text=True).stdout.strip().splitlines()[-1].split()
    os.remove(path)
    emit(out, {"step": "save_load", "size": name, "file_bytes": size, "rows": info["rows"],
               "save_s": save_s, "save_gb_per_s": size / save_s / 1e9, "second_save_s": save2_s,
               "staged_d2h_gb_per_s_of_host_rounds": 51.0,
               "load_s": load_s, "load_gb_per_s": size / load_s / 1e9, "of_which_host_verify_s": verify_s,
               "staged_h2d_gb_per_s_of_host_rounds": 56.6,
               "replay_first_round_s": replay1_s, "replay_whole_history_s": replay_s,
               "load_vs_replay": load_s / replay_s, "same_state": same,
               "file_system": {"device": df[0], "type": df[1], "dir": a.dir}})


def small_rounds(eng, out, rounds=50, owners=200, per_owner=20):
    """~50 small rounds, every second one a resend: what the log holds and
    what each further round uploads per segment, before and after compact."""
    from evolu_amd.server import SyncServer

    srv = SyncServer(eng, owners)
    parts = []
    for k in range(rounds // 2):
        import bench
        from evolu_amd import synth

        ts_np, owner_np, _ = synth.config3(owners, per_owner, seed_config=100 + k, request=per_owner)
        client = eng.tree_new(owners)
        parts.append(bench.e2e_bodies(eng, ts_np, owner_np, client))
        client.free()
    for arena, off in parts:
        srv.sync_arena(arena, off)
        srv.sync_arena(arena, off)
    torch.cuda.synchronize()
    before = srv.log_info()
    t0 = time.perf_counter()
    srv.sync_arena(*parts[0])
    round_before = time.perf_counter() - t0
    before = srv.log_info()
    srv.compact()
    after = srv.log_info()
    t0 = time.perf_counter()
    srv.sync_arena(*parts[0])
    round_after = time.perf_counter() - t0
    srv.close()
    emit(out, {"step": "small_rounds", "rounds": 2 * len(parts) + 1, "owners": owners, "per_owner": per_owner,
               "segments_before": before["segments"], "segments_after": after["segments"],
               "rows_before": before["rows"], "rows_after": after["rows"],
               "log_bytes_before": log_bytes(before), "log_bytes_after": log_bytes(after),
               "descriptor_upload_per_round_before": SEG_DESCRIPTOR_BYTES * (before["segments"] + 1),
               "descriptor_upload_per_round_after": SEG_DESCRIPTOR_BYTES * (after["segments"] + 1),
               "next_round_ms_before": round_before * 1e3, "next_round_ms_after": round_after * 1e3})


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--owners", type=int, default=100_000)
    ap.add_argument("--per-owner", type=int, default=1000)
    ap.add_argument("--small-owners", type=int, default=2000)
    ap.add_argument("--small-per-owner", type=int, default=100)
    ap.add_argument("--resend", type=float, default=0.45, help="share of the bodies sent again (all dead rows)")
    ap.add_argument("--dir", default="/tmp", help="where the snapshot file is written")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from evolu_amd.engine import Engine

    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    eng = Engine(0)
    small_rounds(eng, a.out)
    # (one small pass first also warms the context: pinned staging chunks, device blocks)
    measure(eng, a, a.small_owners, a.small_per_owner, a.out)
    if a.owners:
        measure(eng, a, a.owners, a.per_owner, a.out)
    eng.close()


if __name__ == "__main__":
    main()
