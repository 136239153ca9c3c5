"""SyncServer#compact / #save / SyncServer.load / #logInfo of js/evolu_evm.js
through the N-API addon on the GPU, driven from node (js/test_snapshot.js):
bodies, compact + save, a fresh load into a larger store, more bodies --
every answer equals the oracle's ServerDb.sync (index.ts:204-251) of the
whole sequence, as if the server had never restarted."""
import base64
import json
import os
import random
import shutil
import subprocess

import pytest

from tests import workloads as W
from tests.test_gpu_napi import _build_addon
from tests.test_gpu_wire import REQ, _expected, _requests

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


@pytest.mark.skipif(shutil.which("node") is None or not os.path.exists("/usr/include/node/node_api.h"),
                    reason="node / N-API headers not present")
def test_js_sync_server_survives_a_restart(tmp_path):
    _build_addon()
    bodies = _requests(14, n_users=10, n_req=70)
    rng = random.Random(6)
    node = W.node_id(rng)
    ts = W.hlc_timestamps(rng, 8, [node])
    bodies.insert(9, b"\x0a\x05ab")  # truncated: parseBody throws
    bodies.insert(50, REQ(messages=[dict(timestamp=t, content=b"after") for t in ts], userId="after-the-restart",
                          nodeId=node, merkleTree="{}").SerializeToString())  # a new user after the load
    before, after = [bodies[:20], bodies[20:40]], [bodies[40:58], bodies[58:]]
    f = tmp_path / "snap.json"
    f.write_text(json.dumps({"users": 10, "usersAfter": 16, "path": str(tmp_path / "server.snap"),
                             "before": [[base64.b64encode(b).decode() for b in c] for c in before],
                             "after": [[base64.b64encode(b).decode() for b in c] for c in after]}))
    run = subprocess.run(["node", os.path.join(ROOT, "js", "test_snapshot.js"), str(f)], check=True,
                         capture_output=True, text=True, timeout=300)
    got = json.loads(run.stdout.strip().splitlines()[-1])
    want = _expected(bodies)
    assert len(got["answers"]) == len(want)
    for i, (g, w) in enumerate(zip(got["answers"], want)):
        if w in ("500", "ParseBodyError"):
            assert g == 500, i
        else:
            assert g is not None and base64.b64decode(g) == w, i
    log = got["log"]
    assert log["before"]["segments"] > 1 and log["before"]["rows"] > log["compacted"]["rows"]
    assert log["compacted"]["segments"] == 1
    assert log["saved"] == log["compacted"] == log["loaded"]
    assert got["damaged"] == "13"  # EVM_ESNAPSHOT
    from evolu_amd.server import snapshot_info

    info = snapshot_info(str(tmp_path / "server.snap"))
    assert (info["rows"], info["content_bytes"], info["blob_bytes"]) == (log["saved"]["rows"],
                                                                         log["saved"]["contentBytes"], 0)
