"""SyncServer#syncAsync, #exportUser and #isHandedOver of js/evolu_evm.js
through the N-API addon on the GPU, driven from node (js/test_sync_async.js),
against the oracle's ServerDb.sync (index.ts:204-251): the rounds run off the
JS thread, in issue order, and a request answered null leaves the device and
the caller's reference database consistent."""
import base64
import json
import os
import random
import shutil
import subprocess

import pytest

from oracle import evolu_oracle as O
from tests import workloads as W
from tests.test_gpu_napi import _build_addon
from tests.test_gpu_sync_handover import answer, expected_export, req, seed
from tests.test_gpu_wire import REQ, _expected, _requests

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def _b64(calls):
    return [[base64.b64encode(b).decode() for b in c] for c in calls]


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    """One node process for the whole module: (cases, its output)."""
    if shutil.which("node") is None or not os.path.exists("/usr/include/node/node_api.h"):
        pytest.skip("node / N-API headers not present")
    _build_addon()
    # ---- the calls of test_js_sync_server_round_equals_server_db
    bodies = _requests(9, n_users=10, n_req=40)
    rng = random.Random(4)
    node = W.node_id(rng)
    ts = W.hlc_timestamps(rng, 6, [node])
    bodies.insert(7, b"\x0a\x05ab")  # truncated: parseBody throws
    bodies.insert(13, REQ(messages=[dict(timestamp=t, content=b"q") for t in ts], userId="no-tree",
                          nodeId=node).SerializeToString())  # merkleTree absent: JSON.parse("") throws
    calls = [bodies[:17], bodies[17:30], bodies[30:]]
    # ---- three calls, user X in all of them: X's last answer holds what the first two stored
    nodes = [W.node_id(rng) for _ in range(3)]
    pool = {u: W.hlc_timestamps(rng, 30, nodes) for u in ["X", "Y", "W", "A", "B", "G"]}
    order = [[req("X", pool["X"][:5], nodes[0]), req("Y", pool["Y"][:4], nodes[0])],
             [req("W", pool["W"][:3], nodes[1]), req("X", pool["X"][5:10], nodes[1]),
              req("X", pool["X"][10:12], nodes[0])],
             [req("X", [], nodes[2]), req("Y", [], nodes[2])]]
    # ---- state safety: A turns lenient, B sends an invalid date
    lenient = "2024-02-30T23:59:59.999Z-000a-" + nodes[1]
    bad_date = "2024-02-32T10:00:00.000Z-0000-" + nodes[1]
    safety = [[req("A", pool["A"][:8], nodes[0]), req("B", pool["B"][:8], nodes[0]), req("G", pool["G"][:8], nodes[0])],
              [req("A", pool["A"][8:10] + [lenient], nodes[0]), req("A", pool["A"][10:14], nodes[1]),
               req("B", pool["B"][8:10] + [bad_date], nodes[1]), req("G", pool["G"][8:12], nodes[1])],
              [req("B", pool["B"][8:12], nodes[2]), req("A", [], nodes[2]), req("G", [], nodes[2])]]
    # ---- overlapping batches: A's null in the first of two calls issued together
    overlap = {"setup": [req("A", pool["A"][:8], nodes[0]), req("G", pool["G"][:8], nodes[0])],
               "first": [req("G", pool["G"][8:10], nodes[1]), req("A", pool["A"][8:10] + [lenient], nodes[0])],
               "second": [req("A", pool["A"][10:14], nodes[1]), req("G", pool["G"][10:14], nodes[2])]}
    never = str(tmp_path_factory.mktemp("napi_async_save") / "never.snap")  # (save() must throw, not write)
    cases = {"users": 16, "calls": _b64(calls), "order": _b64(order),
             "overlap": dict({k: _b64([v])[0] for k, v in overlap.items()}, user="A", path=never),
             "safety": {"calls": _b64(safety), "users": [[REQ.FromString(b).userId for b in c] for c in safety],
                        "ask": ["A", "B", "G", "nobody"]}}
    f = tmp_path_factory.mktemp("napi_async") / "cases.json"
    f.write_text(json.dumps(cases))
    p = subprocess.run(["node", os.path.join(ROOT, "js", "test_sync_async.js"), str(f)], check=True,
                       capture_output=True, text=True, timeout=300)
    made = {"bodies": bodies, "order": order, "safety": safety, "overlap": overlap, "never": never}
    return made, json.loads(p.stdout.strip().splitlines()[-1])


def _same(got, want, where):
    assert len(got) == len(want), where
    for i, (g, w) in enumerate(zip(got, want)):
        if w in ("500", "ParseBodyError"):
            assert g == 500, (where, i)
        else:
            assert g is not None and g != 500 and base64.b64decode(g) == w, (where, i)


def test_sync_async_equals_server_db(run):
    cases, got = run
    _same(got["same"], _expected(cases["bodies"]), "same")


def test_calls_issued_without_awaiting_apply_in_issue_order(run):
    cases, got = run
    flat = [b for c in cases["order"] for b in c]
    _same([g for c in got["order"] for g in c], _expected(flat), "order")
    assert [len(c) for c in got["order"]] == [len(c) for c in cases["order"]]
    # X's empty request in the third call is answered with what the first two calls stored
    assert len(REQ.FromString(flat[0]).messages) == 5
    from tests.test_wire import RESP

    assert len(RESP.FromString(base64.b64decode(got["order"][2][0])).messages) > 5
    assert got["pendingThrows"] is True  # close() with a call pending throws (and closes nothing)


def test_sync_async_leaves_the_event_loop(run):
    """A dozen microtask turns after syncAsync returned its Promise is still
    unsettled: completion needs a turn of the event loop.  The control, a
    blocking sync() wrapped in an async function, is settled by then."""
    _, got = run
    assert got["settledEarly"] is False
    assert got["blockingSettledEarly"] is True


def test_null_means_the_user_is_the_callers(run):
    cases, got = run
    full, dev, ref = O.ServerDb(), O.ServerDb(), O.ServerDb()
    seeded = set()
    kinds = []
    for c, (call, answers) in enumerate(zip(cases["safety"], got["safety"])):
        assert len(call) == len(answers)
        nulls = []
        for b, g in zip(call, answers):
            w = answer(full, b)
            if g is None:
                nulls.append((b, w))
            elif g == 500:
                assert w == "500", c
            else:
                assert base64.b64decode(g) == w, c
                answer(dev, b)
            kinds.append("null" if g is None else 500 if g == 500 else "bytes")
        # the caller's side of INTEGRATION.md's handler: seed once from the export, then the reference handler
        for b, _ in nulls:
            u = REQ.FromString(b).userId
            if u not in seeded:
                exp = base64.b64decode(got["exports"][u])
                assert exp == expected_export(dev, u), u  # what the device held when it let go of the user
                seed(ref, u, exp)
                seeded.add(u)
        # ... which then answers as the database that saw all of the user's traffic from the start
        for b, w in nulls:
            assert answer(ref, b) == w and isinstance(w, bytes), c
    # call 1: A's lenient request and the one after it in the same call are both the caller's (the
    # second was not applied on the device: the export above holds call 0's rows only); B's invalid
    # date answers 500 and B is served afterwards
    assert kinds == ["bytes"] * 3 + ["null", "null", 500, "bytes"] + ["bytes", "null", "bytes"]
    assert seeded == {"A"} and set(got["exports"]) == {"A"}
    assert got["handed"] == {"A": True, "B": False, "G": False, "nobody": None}
    assert got["exportUnknown"] is None


def test_export_from_a_continuation_while_another_call_is_pending(run):
    """INTEGRATION.md's handler under overlapping batches: the first call's
    continuation exports the user it was answered null for while the second
    call, issued before the first was awaited, is still pending."""
    cases, got = run
    ov, o = cases["overlap"], got["overlap"]
    full, dev = O.ServerDb(), O.ServerDb()
    for b in ov["setup"]:
        answer(full, b)
        answer(dev, b)
    want_first = [answer(full, b) for b in ov["first"]]
    answer(dev, ov["first"][0])
    assert o["first"][1] is None and base64.b64decode(o["first"][0]) == want_first[0]
    # both exports were taken with the second call pending: at once (its round not yet queued) and a
    # few microtask turns later (its round in flight or queued); both are what the device held for A
    assert o["secondSettledAtExport"] == [False, False]
    want_export = expected_export(dev, "A")
    assert [base64.b64decode(e) for e in o["exports"]] == [want_export, want_export]
    assert o["handed"] == [True, True] and o["rows"] >= 16
    assert o["throws"] == {"close": True, "save": True, "compact": True, "sync": True, "engineClose": True}
    assert not os.path.exists(cases["never"]) and not os.path.exists(cases["never"] + ".tmp")
    # the second call: A's request is the caller's (not applied: the export is unchanged), G is served
    want_second = [answer(full, b) for b in ov["second"]]
    assert o["second"][0] is None and base64.b64decode(o["second"][1]) == want_second[1]
    assert base64.b64decode(o["exportAfter"]) == want_export
    # ... and the seeded reference database answers A's requests as the one that saw everything
    ref = O.ServerDb()
    seed(ref, "A", want_export)
    assert answer(ref, ov["first"][1]) == want_first[1] and answer(ref, ov["second"][0]) == want_second[0]
