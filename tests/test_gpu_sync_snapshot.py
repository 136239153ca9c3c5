"""SyncServer.save / SyncServer.load (evm_sync_save, evm_sync_load): the server
written to one file and read back into a new store -- the directory, the
hand-over flags, the compacted message log, the store rebuilt by ingesting
the saved rows (ids as saved), the owners' roots as the integrity check, and
the Python class's own state in the blob.  A loaded server answers later
calls byte for byte like a twin that never restarted and like the oracle's
ServerDb.sync of the whole history."""
import ctypes as C
import os
import random
import struct

import numpy as np
import pytest

from tests import workloads as W
from tests.test_gpu_wire import _expected, _requests
from tests.test_snapshot_host import GOLDEN, GOLDEN_COUNTS, damaged, resum, sections
from tests.test_wire import REQ

pytestmark = pytest.mark.gpu

CAPACITY = 24


@pytest.fixture(scope="module")
def eng():
    from evolu_amd.engine import Engine

    e = Engine(0)
    yield e
    e.close()


def _req(u, ts, node, contents=None, tree="{}"):
    msgs = [dict(timestamp=t, content=(contents[k] if contents else b"c%d" % k)) for k, t in enumerate(ts)]
    return REQ(messages=msgs, userId=u, nodeId=node, merkleTree=tree).SerializeToString()


class History:
    """Bodies over ~17 users: mixed rounds with redeliveries, a row under a
    lenient spelling (per-request path, kept raw), a user handed over."""

    def __init__(self, seed=5):
        rng = random.Random(seed)
        self.nodes = [W.node_id(rng) for _ in range(3)]
        self.pool = W.hlc_timestamps(rng, 60, self.nodes)
        self.raw = "2024-02-30T23:59:59.999Z-000a-" + self.nodes[1]
        self.mixed = _requests(seed + 300, n_users=14, n_req=90)
        self.users = sorted({REQ.FromString(b).userId for b in self.mixed})
        self.bodies = (self.mixed[:60]
                       + [_req("lenny", self.pool[:6] + [self.raw], self.nodes[1]),
                          _req("dora", self.pool[6:9], "not-a-node"),  # handed over, unapplied
                          _req("big", self.pool[9:12], self.nodes[0], [b"", bytes(range(256)) * 17, b"x"])]
                       + self.mixed[60:])

    def more(self, seed):
        """Later bodies: the mixed users again, the lenient user, the handed-over user, a new user."""
        out = []
        for k, b in enumerate(_requests(seed, n_users=8, n_req=40)):
            r = REQ.FromString(b)
            out.append(REQ(messages=r.messages, userId=self.users[k % len(self.users)], nodeId=r.nodeId,
                           merkleTree=r.merkleTree).SerializeToString())
        out.insert(5, _req("lenny", self.pool[4:8] + [self.raw], self.nodes[2]))
        out.insert(9, _req("dora", self.pool[6:9], self.nodes[0]))
        out.insert(11, _req("newcomer", self.pool[20:25], self.nodes[0]))
        out.append(_req("big", [], self.nodes[1]))
        return out


def _same(got, twin, want):
    assert len(got) == len(twin) == len(want)
    for i, (g, t, w) in enumerate(zip(got, twin, want)):
        if isinstance(g, (bytes, type(None))):
            assert g == t, i
        else:
            assert type(g) is type(t), (i, g, t)
        if isinstance(g, bytes):
            assert g == w, i
    assert sum(isinstance(g, bytes) for g in got) >= len(got) - 2


def _trees(srv):
    tree = srv.store.tree()
    return {u: tree.to_json(s) for u, s in srv.slot.items()}


def _state(srv):
    return dict(slot=srv.slot, detached=set(srv.detached), lenient=dict(srv.lenient), raw=dict(srv._raw),
                next_id=srv.next_id, trees=_trees(srv), n=srv.store.n_messages, log=srv.log_info())


def _raw_load(eng, store, path):
    """evm_sync_load through ctypes -> (status, server handle)."""
    from evolu_amd import _lib

    h, n = C.c_void_p(), C.c_uint64()
    blob = np.zeros(1 << 16, dtype=np.uint8)
    st = _lib.load().evm_sync_load(eng.h, store.h, str(path).encode(), C.byref(h), C.c_void_p(blob.ctypes.data),
                                   len(blob), C.byref(n))
    return st, h


@pytest.fixture(scope="module")
def saved(eng, tmp_path_factory):
    """A server run over the history and saved (then closed), its state at the
    save, and a twin that never restarts."""
    from evolu_amd.server import SyncServer

    hist = History()
    srv, twin = SyncServer(eng, CAPACITY), SyncServer(eng, CAPACITY)
    got, got_twin = srv.sync(hist.bodies), twin.sync(hist.bodies)
    _same(got, got_twin, _expected(hist.bodies))
    assert "dora" in srv.detached and "lenny" in srv.lenient and srv.log_info()["segments"] > 1
    path = str(tmp_path_factory.mktemp("snap") / "server.snap")
    srv.save(path)
    assert not os.path.exists(path + ".tmp")
    state = _state(srv)
    assert state["log"]["segments"] == 1 and state["next_id"] == state["n"] == state["log"]["rows"]
    assert state["trees"] == _trees(twin)
    srv.close()
    twin.close()
    yield dict(hist=hist, path=path, state=state)


@pytest.mark.parametrize("capacity", [CAPACITY, 3 * CAPACITY + 1])
def test_round_trip(eng, saved, capacity):
    from evolu_amd.server import SyncServer, snapshot_info

    info = snapshot_info(saved["path"])
    assert (info["users"], info["rows"]) == (len(saved["state"]["slot"]), saved["state"]["n"])
    srv = SyncServer.load(eng, saved["path"], capacity)
    assert srv.capacity == capacity and _state(srv) == saved["state"]
    # later calls: the loaded server, a twin that never restarted, the oracle
    hist = saved["hist"]
    more = hist.more(900 + capacity)
    twin = SyncServer(eng, CAPACITY)
    twin.sync(hist.bodies)
    before = twin.sync(more)
    twin.close()
    got = srv.sync(more)
    _same(got, before, _expected(hist.bodies + more)[len(hist.bodies):])
    assert got[9] is None and "dora" in srv.detached  # the hand-over flag came back
    assert isinstance(got[5], bytes) and hist.raw.encode() in got[5]  # and the raw spelling
    assert isinstance(got[11], bytes) and "newcomer" in srv.slot
    assert srv.slot["newcomer"] == len(saved["state"]["slot"])  # (new users take the next slot)
    srv.close()


def test_default_capacity_is_the_saved_users(eng, saved):
    from evolu_amd.server import SyncServer

    srv = SyncServer.load(eng, saved["path"])
    assert srv.capacity == len(saved["state"]["slot"]) and _state(srv) == saved["state"]
    srv.close()


def test_saves_are_deterministic(eng, saved, tmp_path):
    """Two saves of one state, and a save of the loaded state, are byte-equal."""
    from evolu_amd.server import SyncServer

    good = open(saved["path"], "rb").read()
    srv = SyncServer.load(eng, saved["path"], 2 * CAPACITY)
    a, b = str(tmp_path / "a.snap"), str(tmp_path / "b.snap")
    srv.save(a)
    srv.save(b)
    srv.close()
    assert open(a, "rb").read() == good and open(b, "rb").read() == good


def test_save_needs_a_compact_log(eng, tmp_path):
    from evolu_amd import _lib
    from evolu_amd.server import SyncServer

    hist = History()
    srv = SyncServer(eng, CAPACITY)
    srv.sync(hist.bodies[:40])
    assert srv.log_info()["segments"] > 1
    path = str(tmp_path / "x.snap")
    lib = _lib.load()
    assert lib.evm_sync_save(srv.h, path.encode(), None, 0) == _lib.EVM_ESTATE
    assert not os.path.exists(path) and not os.path.exists(path + ".tmp")
    srv.compact()
    assert lib.evm_sync_save(srv.h, path.encode(), None, 0) == _lib.EVM_OK
    assert os.path.exists(path) and not os.path.exists(path + ".tmp")
    srv.close()


def test_load_preconditions(eng, saved):
    from evolu_amd import _lib

    users = len(saved["state"]["slot"])
    small = eng.store_new(users - 1)
    st, _ = _raw_load(eng, small, saved["path"])
    assert st == _lib.EVM_ECAPACITY and small.n_messages == 0
    small.free()
    full = eng.store_new(CAPACITY)
    ts = eng.timestamps(saved["hist"].pool[:4])
    full.ingest(ts, eng.dev(np.zeros(4, dtype=np.uint32)))
    st, _ = _raw_load(eng, full, saved["path"])
    assert st == _lib.EVM_EINVAL and full.n_messages == 4
    full.free()


def test_damaged_files_never_reach_the_device(eng, saved, tmp_path):
    """Every damaged file answers EVM_ESNAPSHOT from the host's verification:
    not one kernel is launched for any of them (the engine's kernel profile
    stays empty), the store stays empty and usable."""
    from evolu_amd import _lib
    from evolu_amd.server import SyncServer

    good = open(saved["path"], "rb").read()
    cases = damaged(good)
    assert {what.split(" in ")[-1] for what, _ in cases if what.startswith("flip in ")} >= set(
        n for n, _, ln in sections(good) if ln)
    store = eng.store_new(CAPACITY)
    p = tmp_path / "bad.snap"
    eng.prof_reset()
    eng.prof_enable(True)
    try:
        for what, data in cases:
            p.write_bytes(data)
            st, h = _raw_load(eng, store, p)
            assert st == _lib.EVM_ESNAPSHOT and not h.value, what
        launched = eng.prof_report()
    finally:
        eng.prof_enable(False)
        eng.prof_reset()
    assert launched == {}
    assert store.n_messages == 0
    st, h = _raw_load(eng, store, saved["path"])
    assert st == _lib.EVM_OK and store.n_messages == saved["state"]["n"]
    assert _lib.load().evm_sync_destroy(h) == _lib.EVM_OK
    store.free()
    # (the Python loader reports the same status)
    p.write_bytes(cases[3][1])
    with pytest.raises(_lib.EngineError) as e:
        SyncServer.load(eng, str(p))
    assert e.value.status == _lib.EVM_ESNAPSHOT


def test_altered_root_is_caught_after_the_rebuild(eng, saved, tmp_path):
    """Checksums that hold do not make a file true: one owner's saved root
    altered (its section re-summed) passes the host's verification, and the
    rebuilt store's roots, compared on the device, reject it -- the store is
    emptied again."""
    from evolu_amd import _lib
    from evolu_amd.server import snapshot_info

    good = open(saved["path"], "rb").read()
    sec = {name: (at, ln) for name, at, ln in sections(good)}
    users = len(saved["state"]["slot"])
    owner = saved["state"]["slot"][saved["hist"].users[3]]
    store = eng.store_new(CAPACITY)
    p = tmp_path / "roots.snap"
    for what in ("root", "present"):
        b = bytearray(good)
        if what == "root":
            at = sec["roots"][0] + 4 * owner
            (r,) = struct.unpack_from("<i", b, at)
            struct.pack_into("<i", b, at, r ^ 0x40)
        else:
            b[sec["roots"][0] + 4 * users + owner] ^= 1
        p.write_bytes(resum(b, "roots"))
        assert snapshot_info(str(p))["users"] == users  # (the host has nothing to object to)
        st, h = _raw_load(eng, store, p)
        assert st == _lib.EVM_ESNAPSHOT and not h.value, what
        assert store.n_messages == 0
        roots, present = store.tree().roots()
        assert not present.any()
    st, h = _raw_load(eng, store, saved["path"])
    assert st == _lib.EVM_OK and store.n_messages == saved["state"]["n"]
    assert _lib.load().evm_sync_destroy(h) == _lib.EVM_OK
    store.free()


# ---- the golden snapshot of tests/test_snapshot_host.py
def golden_server(eng):
    """A handful of users, a few KB: resent rows, a row kept under a lenient
    spelling, a user handed over, contents of 0 .. 4,000 bytes."""
    from evolu_amd.server import SyncServer

    rng = random.Random(2024)
    nodes = [W.node_id(rng) for _ in range(2)]
    pool = W.hlc_timestamps(rng, 40, nodes)
    raw = "2024-02-30T23:59:59.999Z-000a-" + nodes[1]
    lens = [3, 0, 1, 15, 16, 17, 40]
    content = lambda k: bytes((7 * k + j) & 0xFF for j in range(lens[k % len(lens)]))  # noqa: E731
    bodies = [_req("alice", pool[:12], nodes[0], [content(k) for k in range(12)]),
              _req("bob", pool[12:24], nodes[1], [content(k + 3) for k in range(12)]),
              _req("alice", pool[6:18], nodes[1], [content(k + 1) for k in range(12)]),  # six resent, six new
              _req("carol", pool[24:29], nodes[0], [b"", bytes(range(250)) * 16, b"z", b"", b"yy"]),
              _req("lenny", pool[30:34] + [raw], nodes[1], [content(k) for k in range(5)]),
              _req("dora", pool[35:38], "not-a-node")]
    srv = SyncServer(eng, 8)
    srv.sync(bodies)
    return srv


def test_golden_snapshot_is_what_the_device_writes(eng, tmp_path):
    """The committed golden file, byte for byte, from the device today."""
    from evolu_amd.server import snapshot_info

    srv = golden_server(eng)
    path = str(tmp_path / "golden.snap")
    srv.save(path)
    srv.close()
    assert snapshot_info(path) == GOLDEN_COUNTS
    assert open(path, "rb").read() == open(GOLDEN, "rb").read()
