"""SyncServer.compact (evm_sync_compact): the message log reduced on the
device to the rows the store holds, in one segment, ids renumbered in order.

A server and a twin get the same bodies; only the server is compacted.  The
history has more log rows than one tile of the scan primitive (4,096), in
many segments: native rounds, segments of the per-request path
(evm_sync_log_add), a round whose every row is dead (a pure resend, with
other content bytes), a round whose every row is live, a round with one
request outside the native domain (a short timestamp) beside committed ones.
Content lengths cover 0, 1, 15, 16, 17, 40 and 5,000 bytes.  Afterwards every
answer -- host rounds, a device round, a per-request lenient case -- is
byte-identical to the twin's and to the oracle's ServerDb.sync of the whole
history."""
import random

import numpy as np
import pytest

from tests import workloads as W
from tests.test_gpu_wire import _expected, _requests
from tests.test_wire import REQ

pytestmark = pytest.mark.gpu

LENS = [0, 1, 15, 16, 17, 40]
BIG = 5000
CAPACITY = 80
GONE = None


@pytest.fixture(scope="module")
def eng():
    from evolu_amd.engine import Engine

    e = Engine(0)
    yield e
    e.close()


class History:
    """Calls of SyncRequest bodies (each call one or more native rounds)."""

    def __init__(self, seed, first_dead, last_dead):
        rng = self.rng = random.Random(seed)
        self.nodes = [W.node_id(rng) for _ in range(4)]
        self.own = ["%021x" % rng.getrandbits(84) for _ in range(8)]
        self.pools = {u: W.hlc_timestamps(rng, 330, self.nodes) for u in self.own + ["lenient-user"]}
        self.lenient_ts = "2024-02-30T23:59:59.999Z-000a-" + self.nodes[1]
        own, pools, req = self.own, self.pools, self.req
        calls = []
        first = [req(u, pools[u][:100], big=(u == own[0])) for u in own]
        if first_dead:
            # 46 bytes but no date: the round takes its rows into the segment (ids 0..), its owner commits nothing
            first.insert(0, req("bad-date", ["2024-02-32T10:00:00.000Z-0000-" + self.nodes[1]] + pools[own[0]][:3]))
        calls.append(first)
        self.mixed = _requests(seed + 1000, n_users=60, n_req=380)  # several rounds per user, redeliveries
        calls.append(self.mixed)
        calls.append([req(u, pools[u][:100], salt=1) for u in own])  # a pure resend: every row dead
        calls.append([req(u, pools[u][100:200]) for u in own])  # every row live
        # one request outside the native domain (a short timestamp) beside committed ones
        calls.append([req(u, pools[u][200:250]) for u in own[:4]] + [req("short-ts", ["2024-01-01T00:00:00.000Z-0000-abc"])]
                     + [req(u, pools[u][200:250]) for u in own[4:]])
        # the per-request path (evm_sync_log_add): a lenient spelling, kept raw
        calls.append([req("lenient-user", pools["lenient-user"][:5] + [self.lenient_ts])])
        if last_dead:
            calls.append([req(u, pools[u][100:200], salt=2) for u in own])
        else:
            calls.append([req(u, pools[u][250:330]) for u in own])
        self.calls = calls

    def req(self, u, ts, tree="{}", node=None, big=False, salt=0):
        rng = self.rng
        msgs = [dict(timestamp=t, content=bytes(rng.getrandbits(8) for _ in range(LENS[(k + salt) % len(LENS)])))
                for k, t in enumerate(ts)]
        if big:
            msgs[1]["content"] = bytes(rng.getrandbits(8) for _ in range(BIG))
        return REQ(messages=msgs, userId=u, nodeId=node or self.nodes[0], merkleTree=tree).SerializeToString()

    def more_mixed(self, seed):
        """Further bodies of the users the mixed call introduced."""
        users = sorted({REQ.FromString(b).userId for b in self.mixed})
        out = []
        for k, b in enumerate(_requests(seed, n_users=12, n_req=60)):
            r = REQ.FromString(b)
            out.append(REQ(messages=r.messages, userId=users[k % len(users)], nodeId=r.nodeId,
                           merkleTree=r.merkleTree).SerializeToString())
        return out


class Answers:
    """The server's and the twin's answers call by call, checked against one
    oracle run of the whole history at the end."""

    def __init__(self, srv, twin):
        self.srv, self.twin, self.done, self.got = srv, twin, [], []

    def sync(self, call, where, how=lambda s, c: s.sync(c)):
        a, b = how(self.srv, call), how(self.twin, call)
        assert len(a) == len(b) == len(call)
        for i, (g, t) in enumerate(zip(a, b)):
            # byte answers and hand-overs (None) equal the twin's; an exception object is of the twin's kind
            if isinstance(g, (bytes, type(None))):
                assert g == t, (where, i)
            else:
                assert type(g) is type(t), (where, i, g, t)
        self.done += call
        self.got += [(where, g) for g in a]
        return a

    def check_oracle(self):
        want = _expected(self.done)
        assert len(want) == len(self.got)
        for i, ((where, g), w) in enumerate(zip(self.got, want)):
            if isinstance(g, bytes):
                assert g == w, (where, i)
            elif g is not None:  # (None: a request the engine hands to the caller)
                assert w in ("500", "ParseBodyError"), (where, i)
        assert sum(isinstance(g, bytes) for _, g in self.got) > len(self.got) - 8


@pytest.mark.parametrize("ends", ["dead_ends", "live_ends"])
def test_compact_keeps_every_answer(eng, ends):
    import torch

    from evolu_amd.server import SyncServer

    dead = ends == "dead_ends"
    hist = History(11, first_dead=dead, last_dead=dead)
    srv, twin = SyncServer(eng, CAPACITY), SyncServer(eng, CAPACITY)
    ans = Answers(srv, twin)
    for k, call in enumerate(hist.calls):
        ans.sync(call, "call %d" % k)
    # ---- the history is what the docstring says
    before = srv.log_info()
    rows = before["rows"]
    assert before["segments"] >= 4 and rows >= 5000 and rows == srv.next_id == twin.next_id
    assert len(srv.slot) >= 70
    _, ids = srv.store.messages()
    live = sorted(int(i) for i in ids)
    n = len(live)
    assert n == srv.store.n_messages and len(set(live)) == n and n > 4096
    assert ((0 in live), (rows - 1 in live)) == ((False, False) if dead else (True, True))
    assert rows - n > 1000  # (resends and rolled-back requests)
    # ---- compact, asking where every old id went
    moved = srv.compact(ask=range(rows + 2))
    after = srv.log_info()
    assert after["segments"] == 1 and after["rows"] == n == srv.store.n_messages == srv.next_id
    assert after["content_bytes"] < before["content_bytes"]
    assert twin.log_info() == before  # (the twin is untouched)
    off2, ids2 = srv.store.messages()
    assert sorted(int(i) for i in ids2) == list(range(n))
    assert [moved[i] for i in live] == list(range(n))  # the rank among the live ids: order kept
    assert all(moved[i] is GONE for i in set(range(rows + 2)) - set(live))
    # every live row reads back as the twin's row of the old id (timestamp and content)
    was = twin._messages(live)
    now = srv._messages(list(range(n)))
    assert now == was
    sizes = {len(c) for _, c in now}
    assert set(LENS) | {BIG} <= sizes
    # each owner's rows are the same messages in the same (timestamp) order
    off1, ids1 = twin.store.messages()
    assert (off1 == off2).all() and [moved[int(i)] for i in ids1] == [int(i) for i in ids2]
    # ---- later calls: host rounds, a device round, the per-request lenient path
    more = hist.more_mixed(71)
    ans.sync(more, "host rounds after compact")
    dev = [hist.req(u, hist.pools[u][90:110] + hist.pools[u][320:330], node=hist.nodes[2]) for u in hist.own]
    off = np.zeros(len(dev) + 1, dtype=np.uint64)
    np.cumsum([len(x) for x in dev], out=off[1:])
    arena = torch.zeros(int(off[-1]) + 64, dtype=torch.uint8, device="cuda")
    arena[: int(off[-1])] = torch.from_numpy(np.frombuffer(b"".join(dev), dtype=np.uint8).copy()).cuda()
    ans.sync(dev, "device round after compact", how=lambda s, c: s.sync_device(arena, off).to_host())
    len_req = [hist.req("lenient-user", hist.pools["lenient-user"][3:9] + [hist.lenient_ts], node=hist.nodes[3])]
    a = ans.sync(len_req, "lenient request after compact")
    assert isinstance(a[0], bytes) and hist.lenient_ts.encode() in a[0]
    # ---- compacting again (after the calls above, then at once) ends compact
    srv.compact()
    info = srv.log_info()
    assert info["segments"] == 1 and info["rows"] == srv.store.n_messages
    _, ids3 = srv.store.messages()
    assert srv.compact(ask=[0, info["rows"] - 1, info["rows"]]) == [0, info["rows"] - 1, GONE]  # a no-op
    _, ids4 = srv.store.messages()
    assert (ids3 == ids4).all() and srv.log_info() == info
    ans.sync(more[:20], "after the second compact")
    ans.check_oracle()
    srv.close()
    twin.close()


def test_lenient_raw_spelling_survives_compaction(eng):
    """A row stored under a lenient spelling is answered with its raw string
    (the server's _raw, keyed by message id) before and after its id moves."""
    from evolu_amd.server import SyncServer

    rng = random.Random(3)
    nodes = [W.node_id(rng) for _ in range(2)]
    pool = W.hlc_timestamps(rng, 30, nodes)
    raw = "2024-02-30T23:59:59.999Z-000a-" + nodes[1]

    def req(u, ts, node):
        return REQ(messages=[dict(timestamp=t, content=b"c%d" % k) for k, t in enumerate(ts)], userId=u, nodeId=node,
                   merkleTree="{}").SerializeToString()

    bodies = [req("a", pool[:10], nodes[0]), req("a", pool[:10], nodes[0]), req("l", pool[10:14] + [raw], nodes[1]),
              req("a", pool[5:15], nodes[0])]
    srv = SyncServer(eng, 4)
    assert srv.sync(bodies) == _expected(bodies)
    (old,) = srv._raw
    assert srv.log_info()["segments"] > 1
    srv.compact()
    (new,) = srv._raw
    assert new < old and srv._raw[new] == raw and srv.lenient["l"][next(iter(srv.lenient["l"]))] == (raw, new)
    assert srv._messages([new])[0][0] == raw
    ask = [req("l", [], nodes[0]), req("a", [], nodes[1])]
    got = srv.sync(ask)
    assert got == _expected(bodies + ask)[-2:] and raw.encode() in got[0]
    srv.close()
