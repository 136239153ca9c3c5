"""evm_ts_classify (Engine.classify_timestamps): evolu_amd/lenient.py:classify
on the device, one row per lane, over the 6,000 V8-generated vectors of
tests/golden/js_lenient.json.  Class and canonical bytes equal
lenient.classify; for ok and range_error they equal V8's own answer (the
vector's `canonical`).  No excuse list."""
import json
import os

import numpy as np
import pytest

from evolu_amd import lenient

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VEC = json.load(open(os.path.join(ROOT, "tests", "golden", "js_lenient.json")))["vectors"]
NAMES = ["ok", "range_error", "unsupported"]


@pytest.fixture(scope="module")
def eng():
    from evolu_amd.engine import Engine

    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def want():
    """lenient.classify of every vector, computed once."""
    return [lenient.classify(v["raw"]) for v in VEC]


def _classify(eng, raws, stride):
    """rows at `stride` (the bytes between rows are 0xEE, not part of a row) -> [(class name, canon | None)]"""
    n = len(raws)
    arena = np.full((n, stride), 0xEE, dtype=np.uint8)
    arena[:, :46] = np.frombuffer("".join(raws).encode("ascii"), dtype=np.uint8).reshape(n, 46)
    cls, canon = eng.classify_timestamps(eng.dev(arena))
    cls, canon = cls.cpu().numpy(), canon.cpu().numpy()
    assert cls.shape == (n,) and canon.shape == (n, 46)
    out = []
    for i in range(n):
        assert cls[i] in (0, 1, 2), i
        if cls[i] == 0:
            out.append(("ok", canon[i].tobytes().decode("ascii")))
        else:
            assert not canon[i].any(), i  # (canon is written for EVM_TS_OK rows only)
            out.append((NAMES[cls[i]], None))
    return out


@pytest.mark.parametrize("stride", [46, 48])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 6000])
def test_vectors(eng, want, n, stride):
    # (the short counts start at different vectors so that all three classes appear in them)
    start = {1: 0, 63: 100, 64: 1000, 65: 2000, 6000: 0}[n]
    vec, exp = VEC[start:start + n], want[start:start + n]
    got = _classify(eng, [v["raw"] for v in vec], stride)
    assert len(got) == n
    for v, g, w in zip(vec, got, exp):
        assert g == w, v["raw"]
        if g[0] == "ok":
            assert g[1] == v["canonical"], v["raw"]
        elif g[0] == "range_error":
            assert v["canonical"] == "RangeError", v["raw"]
    if n == 6000:
        assert [sum(g[0] == k for g in got) for k in NAMES] == [1375, 4418, 207]


@pytest.mark.parametrize("stride", [46, 48])
def test_canonical_and_domain_edges(eng, stride):
    node = "0123456789abcDEF"
    canonical = ["1970-01-01T00:00:00.000Z-0000-0000000000000000", "2024-05-17T12:34:56.789Z-00FF-" + node,
                 "6053-01-23T02:07:59.999Z-FFFF-" + node]  # (the last milli below 2^31 minutes)
    outside = ["1969-12-31T23:59:59.999Z-0000-" + node,  # year 1969
               "6053-01-23T02:08:00.000Z-0000-" + node,  # 2^31 minutes
               "9999-12-31T23:59:59.999Z-0000-" + node]
    rolled = {"1969-12-31T24:00:00.000Z-000a-" + node: "1970-01-01T00:00:00.000Z-000A-" + node,
              "2023-02-29t00:00:00.000z-abcd-" + node: "2023-03-01T00:00:00.000Z-ABCD-" + node}
    raws = canonical + outside + list(rolled)
    got = _classify(eng, raws, stride)
    for r, g in zip(raws, got):
        assert g == lenient.classify(r), r
    assert got[:3] == [("ok", c) for c in canonical]  # a canonical row is its own canon
    assert got[3:6] == [("unsupported", None)] * 3
    assert got[6:] == [("ok", c) for c in rolled.values()]
