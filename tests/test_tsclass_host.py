"""The timestamp classifier's arithmetic on the host (no GPU):
evolu_amd/csrc/evm_tsclass.hpp -- the code evm_ts_classify and the sync
round's EVM_SYNC_OPT_DATE_500 run per lane -- compiled into the stand-alone
tools/tsclass_host.cpp, against evolu_amd/lenient.py and V8's own answers
(tests/golden/js_lenient.json).  The tool's header gives the ASan / UBSan
build of the same program."""
import json
import os
import random
import shutil
import subprocess

import pytest

from evolu_amd import lenient

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VEC = json.load(open(os.path.join(ROOT, "tests", "golden", "js_lenient.json")))["vectors"]
CLS = {"ok": 0, "range_error": 1, "unsupported": 2}


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no host compiler")
    out = str(tmp_path_factory.mktemp("tsclass") / "tsclass_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-I" + os.path.join(ROOT, "evolu_amd", "csrc"),
                    os.path.join(ROOT, "tools", "tsclass_host.cpp"), "-o", out], check=True)
    return out


def _run(tool, rows, tmp_path):
    assert all(len(r) == 46 for r in rows)
    f = tmp_path / "rows.bin"
    f.write_bytes(b"".join(rows))
    out = subprocess.run([tool, str(f)], check=True, capture_output=True, timeout=120).stdout
    got = []
    for line in out.decode("latin-1").split("\n")[:-1]:
        got.append((int(line[0]), line[2:] if line[0] == "0" else None))
    assert len(got) == len(rows)
    return got


def _want(raw: bytes):
    kind, canon = lenient.classify(raw.decode("latin-1"))
    return CLS[kind], canon


def test_v8_vectors(tool, tmp_path):
    rows = [v["raw"].encode("ascii") for v in VEC]
    got = _run(tool, rows, tmp_path)
    counts = [0, 0, 0]
    for v, r, g in zip(VEC, rows, got):
        assert g == _want(r), v["raw"]
        counts[g[0]] += 1
        if g[0] == 0:
            assert g[1] == v["canonical"], v["raw"]  # V8's timestampToString(timestampFromString(raw))
        elif g[0] == 1:
            assert v["canonical"] == "RangeError", v["raw"]
    assert counts == [1375, 4418, 207]


def test_edges_and_damaged_rows(tool, tmp_path):
    node = "0123456789abcDEF"
    edges = [
        "1970-01-01T00:00:00.000Z-0000-0000000000000000",  # canonical: its own canon
        "2024-05-17T12:34:56.789Z-00FF-" + node,
        "1969-12-31T23:59:59.999Z-0000-" + node,  # before 1970
        "1969-12-31T24:00:00.000Z-0000-" + node,  # hour 24 rolls into 1970-01-01
        "6053-01-23T02:07:59.999Z-0000-" + node,  # the last milli below 2^31 minutes
        "6053-01-23T02:08:00.000Z-0000-" + node,  # 2^31 minutes
        "6053-01-22T24:00:00.000Z-ffff-" + node,
        "9999-12-31T23:59:59.999Z-0000-" + node,
        "0000-01-01T00:00:00.000Z-0000-" + node,
        "2023-02-29t00:00:00.000z-abcd-" + node,  # rolls into March 1
        "2024-02-29T00:00:00.000Z-abcd-" + node,  # a leap day
        "2100-02-29T00:00:00.000Z-0000-" + node,  # 2100 is no leap year
        "2024-04-31T24:00:00.000Z-0000-" + node,  # both roll
        "2024-12-31T24:00:00.000Z-0000-" + node,  # into the next year
        "2024-00-10T00:00:00.000Z-0000-" + node, "2024-13-10T00:00:00.000Z-0000-" + node,
        "2024-01-00T00:00:00.000Z-0000-" + node, "2024-01-32T00:00:00.000Z-0000-" + node,
        "2024-01-01T25:00:00.000Z-0000-" + node, "2024-01-01T24:00:00.001Z-0000-" + node,
        "2024-01-01T24:01:00.000Z-0000-" + node, "2024-01-01T00:60:00.000Z-0000-" + node,
        "2024-01-01T00:00:60.000Z-0000-" + node,
        "2024-13-01T00:00:00.000Z-000g-" + node,  # the counter is not hex: not modelled, whatever the date
        "2024-01-01 00:00:00.000Z-0000-" + node, "2024-01-01T00:00:00,000Z-0000-" + node,
        "2024-01-01T00:00:00.000Z-0000-" + node[:15] + "g", "2024-01-01T00:00:00.000Z+0000-" + node,
        "+02024-01-01T00:00:00.000Z-00-" + node,
    ]
    rows = [e.encode("ascii") for e in edges]
    rng = random.Random(5)
    alphabet = b"0123456789abcdefABCDEFTtZz-:. \n\x00\xff\xb2g+"
    for v in rng.sample(VEC, 1500):  # one or two bytes of a V8 vector replaced
        r = bytearray(v["raw"].encode("ascii"))
        for _ in range(rng.choice([1, 1, 2])):
            r[rng.randrange(46)] = rng.choice(alphabet)
        rows.append(bytes(r))
    rows += [bytes(rng.getrandbits(8) for _ in range(46)) for _ in range(200)]
    got = _run(tool, rows, tmp_path)
    for r, g in zip(rows, got):
        assert g == _want(r), r
    by = dict(zip(edges, got))
    assert by[edges[0]] == (0, edges[0]) and by[edges[1]] == (0, edges[1])
    assert by[edges[2]][0] == 2 and by[edges[5]][0] == 2 and by[edges[7]][0] == 2
    assert by[edges[6]] == (0, "6053-01-23T00:00:00.000Z-FFFF-" + node)
    assert by[edges[3]] == (0, "1970-01-01T00:00:00.000Z-0000-" + node)
    assert by[edges[4]] == (0, edges[4])
    assert by[edges[9]] == (0, "2023-03-01T00:00:00.000Z-ABCD-" + node)
    assert {g[0] for g in got} == {0, 1, 2}
