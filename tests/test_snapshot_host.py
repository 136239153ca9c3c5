"""The snapshot file's host verifier (evm_snapshot_info, evm_snapshot.cpp) on
the committed golden snapshot: no GPU.  tests/golden/sync_snapshot_v1.bin was
saved on the device by tests/test_gpu_sync_snapshot.py's golden server (which
also checks that the device still writes these bytes).  It pins format
version 1: a change of the layout or the checksum must bump the version.

The layout and the checksum are restated here in Python (from the layout
comment of evm_snapshot.hpp) so that the tests can damage a file precisely
and re-sum a section they altered."""
import os
import struct

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "sync_snapshot_v1.bin")
# the golden server's counts (tests/test_gpu_sync_snapshot.py golden_server)
GOLDEN_COUNTS = {"version": 1, "users": 5, "rows": 40, "content_bytes": 4400, "blob_bytes": 220}

HEADER = 208
SECTIONS = ["klen", "keys", "flags", "owner", "ts", "coff", "content", "roots", "blob"]
_M = (1 << 64) - 1
_K1, _K2 = 0x9E3779B185EBCA87, 0xC2B2AE3D27D4EB4F


def _rotl(x, r):
    return ((x << r) | (x >> (64 - r))) & _M


def sum64(data: bytes) -> int:
    """evm::Sum64 of the bytes."""
    lanes = [0x60EA27EEADC0B5D6, 0x3C6EF372FE94F82B, 0xA54FF53A5F1D36F1, 0x510E527FADE682D1]
    pad = data + b"\0" * (-len(data) % 32)
    words = struct.unpack("<%dQ" % (len(pad) // 8), pad)
    for i in range(0, len(words), 4):
        for k in range(4):
            lanes[k] = (_rotl((lanes[k] + words[i + k] * _K2) & _M, 31) * _K1) & _M
    h = (len(data) * _K2) & _M
    for k in range(4):
        h = (_rotl(h ^ lanes[k], 27) * _K1 + 0x52DCE729) & _M
    h ^= h >> 32
    h = (h * _K2) & _M
    return h ^ (h >> 29)


def sections(data: bytes):
    """[(name, start, length)] of a well-formed file's sections."""
    out, at = [], HEADER
    for k, name in enumerate(SECTIONS):
        (ln,) = struct.unpack_from("<Q", data, 56 + 16 * k)
        out.append((name, at, ln))
        at += ln
    assert at == len(data)
    return out


def resum(data: bytearray, section: str = None) -> bytes:
    """The file with `section`'s checksum (if given) and the header's recomputed."""
    if section is not None:
        k = SECTIONS.index(section)
        _, at, ln = sections(bytes(data))[k]
        struct.pack_into("<Q", data, 64 + 16 * k, sum64(bytes(data[at:at + ln])))
    struct.pack_into("<Q", data, HEADER - 8, sum64(bytes(data[:HEADER - 8])))
    return bytes(data)


def damaged(good: bytes):
    """(what, bytes) of files no load may accept: one byte flipped in the
    header and in each section, the file cut at each section boundary and
    inside each section, bytes appended, and other versions (header re-summed)."""
    out = []
    flip = lambda at: good[:at] + bytes([good[at] ^ 0x20]) + good[at + 1:]  # noqa: E731
    out.append(("flip in the header's counts", flip(17)))
    out.append(("flip in the header's checksum", flip(HEADER - 3)))
    out.append(("flip in the magic", flip(2)))
    for name, at, ln in sections(good):
        if ln:
            out.append(("flip in " + name, flip(at + ln // 2)))
            out.append(("flip at the end of " + name, flip(at + ln - 1)))
            out.append(("cut inside " + name, good[:at + max(ln // 2, 0)] if ln > 1 else good[:at]))
        out.append(("cut before " + name, good[:at]))
    out.append(("cut inside the header", good[:100]))
    out.append(("empty file", b""))
    out.append(("one byte short", good[:-1]))
    out.append(("bytes appended", good + b"\0"))
    for v in (0, 2, 0x01000000):
        b = bytearray(good)
        struct.pack_into("<I", b, 8, v)
        out.append(("version %d" % v, resum(b)))
    return out


def _info(path):
    from evolu_amd.server import snapshot_info

    return snapshot_info(str(path))


def test_sum64_restatement_matches_the_library(tmp_path):
    """The golden file's stored checksums are the library's; the restatement agrees with every one."""
    good = open(GOLDEN, "rb").read()
    for k, (name, at, ln) in enumerate(sections(good)):
        (want,) = struct.unpack_from("<Q", good, 64 + 16 * k)
        assert sum64(good[at:at + ln]) == want, name
    assert sum64(good[:HEADER - 8]) == struct.unpack_from("<Q", good, HEADER - 8)[0]


def test_golden_snapshot_is_accepted():
    assert os.path.getsize(GOLDEN) < 16384
    assert _info(GOLDEN) == GOLDEN_COUNTS
    good = open(GOLDEN, "rb").read()
    assert good[:8] == b"EVMSNAP\0" and struct.unpack_from("<II", good, 8) == (1, len(SECTIONS))
    want = {"klen": 4 * 5, "flags": 5, "owner": 4 * 40, "ts": 48 * 40, "coff": 8 * 41, "content": 4400, "roots": 5 * 5,
            "blob": 220}
    got = {name: ln for name, _, ln in sections(good)}
    assert {k: got[k] for k in want} == want


def test_damaged_snapshots_are_rejected(tmp_path):
    from evolu_amd import _lib

    good = open(GOLDEN, "rb").read()
    cases = damaged(good)
    assert len(cases) > 30
    p = tmp_path / "snap.bin"
    for what, data in cases:
        p.write_bytes(data)
        with pytest.raises(_lib.EngineError) as e:
            _info(p)
        assert e.value.status == _lib.EVM_ESNAPSHOT, what
    with pytest.raises(_lib.EngineError) as e:
        _info(tmp_path / "absent.bin")
    assert e.value.status == _lib.EVM_ESNAPSHOT
    p.write_bytes(good)
    assert _info(p) == GOLDEN_COUNTS


def test_values_the_device_would_trust_are_checked_on_the_host(tmp_path):
    """Valid checksums are not enough: content offsets that do not ascend, an
    owner past the users, key lengths that do not add up and a flag that is
    not 0 / 1 are rejected before any load could send them to the device."""
    from evolu_amd import _lib

    good = open(GOLDEN, "rb").read()
    sec = {name: (at, ln) for name, at, ln in sections(good)}
    p = tmp_path / "snap.bin"

    def put(section, offset, fmt, value):
        b = bytearray(good)
        struct.pack_into(fmt, b, sec[section][0] + offset, value)
        return resum(b, section)

    cases = [("coff descends", put("coff", 8 * 3, "<Q", 0)),
             ("coff past the contents", put("coff", 8 * 40, "<Q", 4401)),
             ("coff does not start at 0", put("coff", 0, "<Q", 1)),
             ("owner past the users", put("owner", 4 * 7, "<I", 5)),
             ("key lengths too long", put("klen", 0, "<I", 1000)),
             ("key lengths too short", put("klen", 4, "<I", 0)),
             ("flag 2", put("flags", 1, "<B", 2))]
    for what, data in cases:
        p.write_bytes(data)
        with pytest.raises(_lib.EngineError) as e:
            _info(p)
        assert e.value.status == _lib.EVM_ESNAPSHOT, what
    # (re-summing an unchanged file changes nothing: the restatement is the library's sum)
    assert resum(bytearray(good), "coff") == good
