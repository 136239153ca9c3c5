"""The sync round's two options and evm_sync_export, on the C ABI (ctypes).

EVM_SYNC_OPT_DATE_500: a rejected request with a row whose date Date.parse
rejects answers EVM_EDATE (the reference's 500, nothing stored, no hand-over).
EVM_SYNC_OPT_HANDOVER: a request answered EVM_ENONCANON flags its user inside
the round; from the next round on that user answers EVM_EHANDOVER.
evm_sync_export: a user's stored tree and rows as a SyncResponse -- what a
caller seeds its reference database with before it runs that user there.

Beside the server run oracle ServerDbs (index.ts:204-251): `full` sees every
request, `dev` only those the device answered (what the device must hold)."""
import ctypes as C
import random

import numpy as np
import pytest

from oracle import evolu_oracle as O
from tests import workloads as W
from tests.test_wire import REQ, RESP

pytestmark = pytest.mark.gpu

ZERO_ROW = "1970-01-01T00:00:00.000Z-0000-0000000000000000"
SELECT_USER = 'SELECT "timestamp", "content" FROM "message" WHERE "userId" = ? ORDER BY "timestamp"'


@pytest.fixture(scope="module")
def eng():
    from evolu_amd.engine import Engine

    e = Engine(0)
    yield e
    e.close()


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


class Srv:
    """evm_sync_* by ctypes: one store, one server."""

    def __init__(self, eng, cap, options=None):
        from evolu_amd import _lib

        self.L, self.lib, self.eng = _lib, _lib.load(), eng
        self.store = eng.store_new(cap)
        self.h = C.c_void_p()
        _lib.check(self.lib.evm_sync_create(eng.h, self.store.h, C.byref(self.h)), "evm_sync_create")
        for opt, v in (options or {}).items():
            _lib.check(self.lib.evm_sync_set_option(self.h, opt, v), "evm_sync_set_option")

    def close(self):
        self.lib.evm_sync_destroy(self.h)
        self.store.free()

    def _fetch(self, roff, total):
        buf = np.zeros(max(total, 1), dtype=np.uint8)
        self.L.check(self.lib.evm_sync_fetch(self.h, _p(buf)), "evm_sync_fetch")
        return [buf[int(roff[k]):int(roff[k + 1])].tobytes() for k in range(len(roff) - 1)]

    def round(self, bodies):
        """-> (per-request codes, per-request response bytes (b"" unless the code is EVM_OK))"""
        n = len(bodies)
        off = np.zeros(n + 1, dtype=np.uint64)
        np.cumsum([len(b) for b in bodies], out=off[1:])
        arena = np.frombuffer(b"".join(bodies) + b"\0" * 16, dtype=np.uint8).copy()
        res, roff, total = np.zeros(n, dtype=np.int32), np.zeros(n + 1, dtype=np.uint64), C.c_uint64()
        self.L.check(self.lib.evm_sync_round(self.h, _p(arena), _p(off), n, self.L.SYNC_HOST, _p(res), _p(roff),
                                             C.byref(total)), "evm_sync_round")
        return [int(c) for c in res], self._fetch(roff, total.value)

    def export_status(self, slots):
        sl = np.asarray(slots, dtype=np.uint32)
        roff, total = np.zeros(len(sl) + 1, dtype=np.uint64), C.c_uint64()
        st = self.lib.evm_sync_export(self.h, _p(sl), len(sl), _p(roff), C.byref(total))
        return st, roff, total.value

    def export(self, slots):
        st, roff, total = self.export_status(slots)
        self.L.check(st, "evm_sync_export")
        assert int(roff[-1]) == total
        return self._fetch(roff, total)

    def slot(self, user):
        """The user's slot, None for a user the directory does not hold."""
        key = np.frombuffer(user.encode() or b"\0", dtype=np.uint8).copy()
        off = np.array([0, len(user.encode())], dtype=np.uint64)
        out = np.zeros(1, dtype=np.uint32)
        self.L.check(self.lib.evm_sync_users(self.h, _p(key), _p(off), 1, 0, _p(out)), "evm_sync_users")
        return None if out[0] == 0xFFFFFFFF else int(out[0])

    def flag(self, user):
        f = C.c_int(-1)
        self.L.check(self.lib.evm_sync_user_flag_get(self.h, self.slot(user), C.byref(f)), "evm_sync_user_flag_get")
        return f.value

    def users(self):
        n = C.c_uint32()
        self.L.check(self.lib.evm_sync_user_count(self.h, C.byref(n), None), "evm_sync_user_count")
        return n.value

    def compact(self):
        self.L.check(self.lib.evm_sync_compact(self.h, None, 0, None), "evm_sync_compact")


def req(user, ts, node, tree="{}", tag=b"c"):
    return REQ(messages=[dict(timestamp=t, content=tag + b"%d" % k if k % 3 else b"") for k, t in enumerate(ts)],
               userId=user, nodeId=node, merkleTree=tree).SerializeToString()


def answer(sdb, body):
    """ServerDb.sync of one body -> the SyncResponse bytes, or "500"."""
    r = REQ.FromString(body)
    try:
        tree, _, rows = sdb.sync(r.userId, r.nodeId, r.merkleTree, [(m.timestamp, m.content) for m in r.messages])
    except (O.RangeErrorJS, ValueError):
        return "500"
    return RESP(messages=[dict(timestamp=t, content=c) for t, c in rows],
                merkleTree=O.merkle_tree_to_string(tree)).SerializeToString()


def expected_export(sdb, user):
    """The reference's two tables for `user` (index.ts:64-75) as a SyncResponse."""
    rows = sdb.conn.execute(SELECT_USER, (user,)).fetchall()
    return RESP(messages=[dict(timestamp=t, content=c) for t, c in rows],
                merkleTree=O.merkle_tree_to_string(sdb.get_merkle_tree(user))).SerializeToString()


def seed(sdb, user, exported: bytes):
    """A user's export into a reference database: its rows and its tree, through conn."""
    r = RESP.FromString(exported)
    sdb.conn.executemany('INSERT INTO "message" ("timestamp", "userId", "content") VALUES (?, ?, ?)',
                         [(m.timestamp, user, m.content) for m in r.messages])
    sdb.conn.execute('INSERT OR REPLACE INTO "merkleTree" ("userId", "merkleTree") VALUES (?, ?)',
                     (user, r.merkleTree))


class World:
    """12 users with about 10 rows each, and the requests of the scenario."""

    def __init__(self, seed_):
        rng = random.Random(seed_)
        self.nodes = nodes = [W.node_id(rng) for _ in range(3)]
        self.plain = ["%021x" % rng.getrandbits(84) for _ in range(8)]
        names = self.plain + ["A", "B", "C", "D", "Z"]
        self.pool = {u: W.hlc_timestamps(rng, 30, nodes + [nodes[0].upper()]) for u in names}
        self.lenient = "2024-02-30T23:59:59.999Z-000a-" + nodes[1]  # V8 rolls it into March; a lower-case counter
        self.lenient2 = "2023-04-31t12:00:00.000z-00FF-" + nodes[2]
        self.bad_date = "2024-02-32T10:00:00.000Z-0000-" + nodes[1]
        self.short = "2024-01-01T00:00:00.000Z-0000-" + nodes[0][:15]  # 45 bytes
        pool = self.pool
        # round 1: everybody's first rows; Z holds the row at millis 0; E has no rows at all
        self.setup = [req(u, pool[u][:10], nodes[0]) for u in self.plain + ["A", "B"]]
        self.setup += [req("Z", [ZERO_ROW] + pool["Z"][:4], nodes[1]), req("E", [], nodes[0])]
        # round 2: the rejected requests beside committed ones
        self.a_lenient = req("A", pool["A"][10:12] + [self.lenient], nodes[0])
        self.b_invalid = req("B", pool["B"][10:13] + [self.bad_date] + pool["B"][13:15], nodes[0])
        self.c_invalid = req("C", [self.bad_date], nodes[1])  # a new user whose first request is the invalid one
        self.d_both = req("D", [self.lenient2, pool["D"][0], self.bad_date], nodes[2])
        self.f_short = req("F", pool["D"][1:3] + [self.short], nodes[2])
        self.mixed = ([req(u, pool[u][10:14], nodes[1]) for u in self.plain[:4]]
                      + [self.a_lenient, self.b_invalid, self.c_invalid, self.d_both, self.f_short]
                      + [req(u, pool[u][10:14], nodes[1]) for u in self.plain[4:]])
        # round 3 on: the same users again
        self.a_later = [req("A", pool["A"][12:16], nodes[1]), req("A", [], nodes[2]),
                        req("A", pool["A"][16:18] + [self.lenient], nodes[0])]
        self.later = [self.a_later[0], req("B", pool["B"][15:19], nodes[1]), req("C", pool["C"][:5], nodes[0]),
                      req("D", pool["D"][3:8], nodes[0]), req(self.plain[0], pool[self.plain[0]][14:18], nodes[2])]


def _run(srv, bodies, full, dev):
    """One round; every answered request equals the oracle's bytes.  -> codes"""
    codes, resp = srv.round(bodies)
    for k, (b, c) in enumerate(zip(bodies, codes)):
        w = answer(full, b) if full is not None else None
        if c == 0:
            answer(dev, b)
            if w is not None:
                assert resp[k] == w, k
        else:
            assert resp[k] == b""
    return codes


def test_options_off_change_nothing(eng):
    from evolu_amd import _lib as L

    w = World(1)
    off = Srv(eng, 16, {L.SYNC_OPT_DATE_500: 0, L.SYNC_OPT_HANDOVER: 0})
    twin = Srv(eng, 16)  # a server that never heard of options
    try:
        for bodies in (w.setup, w.mixed, w.later):
            # the kernels of each round: with the options off a round that rejects requests
            # launches what the twin launches, and neither of the options' kernels
            launched = []
            for srv in (off, twin):
                eng.prof_enable(True)
                eng.prof_reset()
                launched.append((srv.round(bodies), eng.prof_report()))
                eng.prof_enable(False)
            (a, prof_a), (b, prof_b) = launched
            assert a == b
            assert "k_dir_find" in prof_a and not {"k_sync_cls", "k_sync_hand", "k_ts_classify"} & set(prof_a)
            assert {k: v[1] for k, v in prof_a.items()} == {k: v[1] for k, v in prof_b.items()}
            if bodies is w.mixed:
                codes = dict(zip(["A", "B", "C", "D", "F"], a[0][4:9]))
                assert codes == {u: L.EVM_ENONCANON for u in "ABCDF"}  # the lenient and the invalid-date rows alike
        for u in "ABCDF":
            assert off.flag(u) == 0 and twin.flag(u) == 0
        assert off.store.n_messages == twin.store.n_messages
        # an option that does not exist, a value that is no switch
        assert off.lib.evm_sync_set_option(off.h, 3, 1) == L.EVM_EINVAL
        assert off.lib.evm_sync_set_option(off.h, L.SYNC_OPT_HANDOVER, 2) == L.EVM_EINVAL
    finally:
        eng.prof_enable(False)
        off.close()
        twin.close()


def test_options_on_export_and_complete_hand_over(eng):
    from evolu_amd import _lib as L

    w = World(2)
    srv = Srv(eng, 16, {L.SYNC_OPT_DATE_500: 1, L.SYNC_OPT_HANDOVER: 1})
    full, dev = O.ServerDb(), O.ServerDb()
    try:
        # ---- a round that rejects nothing launches nothing new
        eng.prof_enable(True)
        eng.prof_reset()
        assert _run(srv, w.setup, full, dev) == [0] * len(w.setup)
        quiet = eng.prof_report()
        assert "k_dir_find" in quiet and not {"k_sync_cls", "k_sync_hand", "k_ts_classify"} & set(quiet)
        # ---- the rejected requests
        eng.prof_reset()
        before = srv.store.n_messages
        codes = _run(srv, w.mixed, None, dev)
        loud = eng.prof_report()
        eng.prof_enable(False)
        assert loud["k_sync_cls"][1] == 1 and loud["k_sync_hand"][1] == 1
        want = [0] * 4 + [L.EVM_ENONCANON, L.EVM_EDATE, L.EVM_EDATE, L.EVM_EDATE, L.EVM_ENONCANON] + [0] * 4
        assert codes == want  # A lenient; B, C invalid; D invalid beside lenient; F a 45-byte timestamp
        assert srv.store.n_messages == before + 8 * 4  # nothing of the five was stored
        assert [srv.flag(u) for u in "ABCDF"] == [1, 0, 0, 0, 1]  # flagged inside that round; EVM_EDATE flags nobody
        for b, c in zip(w.mixed, codes):  # (F's 45-byte timestamp is not the oracle's business)
            if b is not w.f_short:
                a = answer(full, b)
                assert (a == "500") == (c == L.EVM_EDATE), c
        # ---- export, before anybody touches A again: byte-equal to the reference's tables
        sa, sz, se = srv.slot("A"), srv.slot("Z"), srv.slot("E")
        exp_a = srv.export([sa])[0]
        assert exp_a == expected_export(dev, "A")
        assert len(RESP.FromString(exp_a).messages) == 10 and w.lenient.encode() not in exp_a
        exp_z = srv.export([sz])[0]
        assert exp_z == expected_export(dev, "Z")
        assert RESP.FromString(exp_z).messages[0].timestamp == ZERO_ROW  # not lost to a lower bound
        exp_e = srv.export([se])[0]
        assert exp_e == RESP(merkleTree="{}").SerializeToString() == expected_export(dev, "E")
        batch = srv.export([sa, sz, sa, se, srv.slot("C")])  # a slot twice; C: known, nothing stored
        assert batch == [exp_a, exp_z, exp_a, exp_e, exp_e]
        st, roff, total = srv.export_status([sa, srv.users()])
        assert st == L.EVM_EINVAL and total == 0 and not roff.any()
        assert srv.export([]) == []
        # ---- the next round: A is the caller's; B, C, D are served, byte-equal to ServerDb.sync
        before = srv.store.n_messages
        codes = _run(srv, w.later, full, dev)
        assert codes == [L.EVM_EHANDOVER, 0, 0, 0, 0]
        assert srv.store.n_messages == before + 4 + 5 + 5 + 4  # nothing of A's request
        # ---- export again after compaction (other ids, one segment): the same bytes
        srv.compact()
        assert srv.export([sa, sz]) == [exp_a, exp_z]
        assert srv.export([srv.slot("B")])[0] == expected_export(dev, "B")
        # ---- the hand-over is complete: a reference database seeded from the export answers
        # A's remaining requests as the database that saw all of A's traffic from the start
        ref, whole = O.ServerDb(), O.ServerDb()
        for b in w.setup:
            answer(whole, b)
        seed(ref, "A", exp_a)
        for b in [w.a_lenient] + w.a_later:
            got, want_ = answer(ref, b), answer(whole, b)
            assert got == want_ and isinstance(got, bytes)
        assert expected_export(ref, "A") == expected_export(whole, "A")
        assert w.lenient.encode() in expected_export(ref, "A")
    finally:
        eng.prof_enable(False)
        srv.close()
