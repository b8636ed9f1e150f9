"""CPU: the host maker of the base columns (csrc/bamio.cpp: bam_decode_bases) under AddressSanitizer +
UndefinedBehaviorSanitizer.  `make -C bamsignals_amd/csrc basecols` builds it with tests/asan/basecols_driver.cpp into a
stand-alone program; the hand deck's file and a few hundred seeded damaged copies of it -- a truncated record, an l_seq larger
than its record, an n_cigar_op that runs past its record, a few bytes flipped -- go through it: every file must end in a parse
whose columns fit each other or in a clean error, never in a sanitizer report.  (A CPU build of host code only.)"""
import gzip
import os
import struct
import subprocess
import zlib

import numpy as np

import nucleotides_expected as nx
from conftest import ROOT

DRIVER = os.path.join(ROOT, "tests", "asan", "basecols_driver")
EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def bgzf(data, size=60000):
    out = b""
    for i in range(0, len(data), size):
        chunk = data[i:i + size]
        co = zlib.compressobj(1, zlib.DEFLATED, -15)
        dd = co.compress(chunk) + co.flush()
        out += (b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00" + struct.pack("<H", len(dd) + 25) + dd
                + struct.pack("<II", zlib.crc32(chunk), len(chunk)))
    return out + EOF_BLOCK


def record_starts(stream):
    o = 12 + struct.unpack_from("<i", stream, 4)[0]
    for _ in range(struct.unpack_from("<i", stream, o - 4)[0]):
        o += 8 + struct.unpack_from("<i", stream, o)[0]
    starts = []
    while o + 4 <= len(stream):
        starts.append(o)
        o += 4 + struct.unpack_from("<i", stream, o)[0]
    return starts


def damaged(rng, stream, starts):
    b = bytearray(stream)
    at = starts[int(rng.integers(0, len(starts)))]
    bs = struct.unpack_from("<i", b, at)[0]
    kind = int(rng.integers(0, 5))
    if kind == 0:                   # a truncated record: the stream ends inside it
        del b[at + int(rng.integers(1, 4 + bs)):]
    elif kind == 1:                 # l_seq larger than the record (or negative)
        struct.pack_into("<i", b, at + 20, int(rng.choice([bs, 4 * bs, 1 << 20, 2**31 - 1, -1, -2**31])))
    elif kind == 2:                 # n_cigar_op runs past the record
        struct.pack_into("<H", b, at + 16, int(rng.choice([bs // 4, 65535, 1 + (bs - 32) // 4])))
    elif kind == 3:                 # a block_size that promises less, or more, than the record holds
        struct.pack_into("<i", b, at, int(rng.choice([32, 33, bs - 1, bs + 1, 2**31 - 1])))
    else:                           # a few bytes flipped inside the record
        for _ in range(int(rng.integers(1, 6))):
            b[at + int(rng.integers(0, 4 + bs))] = int(rng.integers(0, 256))
    return bytes(b)


def test_base_columns_of_damaged_files(tmp_path):
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "bamsignals_amd", "csrc"), "basecols"])
    rec, _ = nx.hand_deck()
    # the hand deck without its 70,000 equal reads (the copies stay small): every other shape it plants, the CG tag included
    few = nx.take(rec, np.flatnonzero(~((rec["pos"] == 4000) & (np.diff(rec["seq_off"]) == 3))))
    clean = nx.write_bam(tmp_path / "hand.bam", nx.HAND_NAMES, few)
    stream = gzip.decompress(open(clean, "rb").read())
    starts = record_starts(stream)
    assert len(starts) == len(few["pos"])
    rng = np.random.default_rng(20261021)
    paths = [clean]
    for k in range(300):
        paths.append(str(tmp_path / f"damaged{k}.bam"))
        with open(paths[-1], "wb") as f:
            f.write(bgzf(damaged(rng, stream, starts)))
        with open(paths[-1] + ".bai", "wb") as f:         # (the clean file's index: its offsets may point anywhere now)
            f.write(open(clean + ".bai", "rb").read())
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=66", UBSAN_OPTIONS="print_stacktrace=1", BAMSIGNALS_THREADS="3")
    p = subprocess.run([DRIVER, *paths], capture_output=True, text=True, errors="replace", env=env, timeout=300)
    assert p.returncode == 0, (p.returncode, p.stdout[-400:], p.stderr[-3000:])
    lines = p.stdout.splitlines()
    assert len(lines) == len(paths) and all(ln.startswith(("ok ", "err ")) for ln in lines)
    first = lines[0].split()
    assert first[:3] == ["ok", str(len(few["pos"])), str(len(few["code"]))] and first[3] == first[4], "whole and through the index: the same reads"
    n_err = sum(ln.startswith("err ") for ln in lines)
    assert 0 < n_err < 300, "damage is found, and some of it is harmless"
    assert any("l_seq" in ln for ln in lines) and any("truncated" in ln for ln in lines)
