"""GPU: the inflate kernel on DEFLATE streams zlib's compressor never writes (tests/deflate_writer.py; zlib's inflate is the
reference for every case, tests/test_deflate_writer_cpu.py).  Every stream the kernel met before came out of zlib, and the code
that builds its tables on the device -- coop_cl_table / coop_tables / coop_construct in csrc/inflate_lane.h: ballots, ranks,
the hot symbols' ninth bits OR-ed over the wave, atomicOr into the cold ones -- runs in no host test at all.  Here: more than
128 long symbols with length symbols among the cold ones, cold tables rebuilt inside one BGZF block, distance symbols packed
across both word borders, 15-bit codes with the largest extra bits in one turn, distance 32,768, one distance code and none,
every repeat item at its extremes, dozens of tiny blocks, ISIZE up to 65,536, empty blocks and foreign subfields in the
container -- in all five LANES forms of the kernel (ROUNDS of coop_construct differs in each)."""
import ctypes
import gzip
import struct
import zlib

import pytest

import deflate_writer as dw
from test_device_decode_gpu import BAM, _both_ways, _empty_bai, ctx  # noqa: F401

pytestmark = pytest.mark.gpu

FORMS = (("4", "0"), ("8", "0"), ("16", "100"), ("32", "0"), ("64", "0"), ("32", "288"))     # (LANES, padded LDS)


def _bench(path, first=0, n=1 << 20):
    """k_inflate alone on blocks [first, first + n) of a BGZF file, every block's CRC32 and length checked on the device"""
    from bamsignals_amd import _lib
    fn = _lib.load().bsig_debug_inflate_bench
    fn.argtypes = [ctypes.c_int, ctypes.c_char_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int, ctypes.POINTER(ctypes.c_double),
                   ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int)]
    ms, by, st = (ctypes.c_double * 2)(), (ctypes.c_int64 * 3)(), ctypes.c_int(-1)
    rc = fn(0, str(path).encode(), first, n, 1, ms, by, ctypes.byref(st))
    if rc == 5:                                                        # a HIP error: nothing more goes to this GPU
        pytest.exit("bsig_debug_inflate_bench: HIP error on %s" % path, returncode=3)
    return rc, st.value, by[2], by[1]


@pytest.mark.parametrize("family", dw.FAMILIES)
def test_kernel_alone_on_every_family(ctx, tmp_path, monkeypatch, family):  # noqa: F811
    data, n, total = dw.family_file(family)
    path = tmp_path / "f.bgzf"
    path.write_bytes(data)
    assert len(gzip.decompress(data)) == total and 0 < n <= 300
    for lanes, pad in FORMS:
        monkeypatch.setenv("BAMSIGNALS_INFLATE_LANES", lanes)
        monkeypatch.setenv("BAMSIGNALS_INFLATE_LDS_PAD", pad)
        assert _bench(path) == (0, 0, n, total), (family, lanes, pad)


SPECIAL = ("flat_long/twice", "deep/deep", "few_distance_codes/one_at_symbol_1")


@pytest.mark.parametrize("lanes", [4, 8, 16, 32, 64])
def test_placement_among_ordinary_blocks(ctx, tmp_path, monkeypatch, lanes):  # noqa: F811
    """The wave builds one lane's tables at a time and lanes that are done keep helping: the same three blocks alone in a
    launch, as lane 0, as the last lane of a workgroup and as the first of the next among zlib's level-6 blocks, in a launch of
    LANES + 1 blocks, and with stored blocks as all their neighbours."""
    monkeypatch.setenv("BAMSIGNALS_INFLATE_LANES", str(lanes))
    corpus = dw.corpus()
    stream = gzip.decompress(open(BAM, "rb").read())[:3000 * (lanes + 6)]
    alone = tmp_path / "alone.bgzf"
    alone.write_bytes(b"".join(dw.bgzf_block(*corpus[s]) for s in SPECIAL) + dw.EOF_BLOCK)
    for k in range(3):
        assert _bench(alone, k, 1) == (0, 0, 1, len(corpus[SPECIAL[k]][1])), (lanes, SPECIAL[k])
    for level in (6, 0):
        for rot in range(3):
            blocks, sizes = [], []
            for k in range(lanes + 6):
                if k in (0, lanes - 1, lanes):
                    raw, data = corpus[SPECIAL[((0, lanes - 1, lanes).index(k) + rot) % 3]]
                else:
                    data = stream[3000 * k:3000 * k + 3000]
                    co = zlib.compressobj(level, zlib.DEFLATED, -15)
                    raw = co.compress(data) + co.flush()
                blocks.append(dw.bgzf_block(raw, data))
                sizes.append(len(data))
            path = tmp_path / ("p%d_%d.bgzf" % (level, rot))
            path.write_bytes(b"".join(blocks) + dw.EOF_BLOCK)
            assert _bench(path) == (0, 0, lanes + 6, sum(sizes)), (lanes, level, rot)
            assert _bench(path, 0, lanes + 1) == (0, 0, lanes + 1, sum(sizes[:lanes + 1])), (lanes, level, rot)


@pytest.mark.parametrize("route", ["streamed", "batches of 3 blocks"])
def test_whole_route_on_a_foreign_bam(ctx, tmp_path, monkeypatch, route):  # noqa: F811
    """a BAM whose blocks no zlib wrote -- matches beyond 32,506, 3-byte matches at any distance, ISIZE up to 65,536, empty blocks
    in the middle, another subfield in front of BC -- inflated by the GPU and decoded on the device == the CPU decode (libdeflate
    or zlib: independent of the lane decoder)"""
    data, _, total = dw.family_file("bam_foreign")
    path = tmp_path / "foreign.bam"
    path.write_bytes(data)
    _empty_bai(str(path) + ".bai", 2)
    monkeypatch.setenv("BAMSIGNALS_INFLATE", "gpu")
    if route == "streamed":
        monkeypatch.setenv("BAMSIGNALS_STREAM_MIN_MB", "0")
        monkeypatch.setenv("BAMSIGNALS_INFLATE_ROUND_BLOCKS", "7")
        monkeypatch.setenv("BAMSIGNALS_STREAM_CHUNK_KB", "100")
    else:
        monkeypatch.setenv("BAMSIGNALS_BATCH_BLOCKS", "3")
    _, dev = _both_ways(ctx, str(path), monkeypatch)
    assert dev.n_reads == dw.BAM_FOREIGN_READS
    dev.close()


@pytest.mark.parametrize("name", dw.TABLE_LEVEL)
def test_invalid_tables_and_symbols_are_reported(ctx, tmp_path, monkeypatch, name):  # noqa: F811
    """streams that fail at their code tables or at a checked symbol, in place of one block of the fixture BAM: k_inflate
    reports it, the call takes the CPU path, which names the problem"""
    from bamsignals_amd import _lib
    from bamsignals_amd.bamio import BamFile
    from bamsignals_amd.device import Reads
    raw = open(BAM, "rb").read()
    o = struct.unpack_from("<H", raw, 16)[0] + 1                       # the second block
    bsize = struct.unpack_from("<H", raw, o + 16)[0] + 1
    crc, isize = struct.unpack_from("<II", raw, o + bsize - 8)
    bad = dw.bgzf_block(dw.invalid()[name][0], b"", crc=crc, isize=isize)
    p = tmp_path / "bad.bam"
    p.write_bytes(raw[:o] + bad + raw[o + bsize:])
    _empty_bai(str(p) + ".bai", 3)
    monkeypatch.setenv("BAMSIGNALS_INFLATE", "gpu")
    monkeypatch.setenv("BAMSIGNALS_DEVICE_DECODE", "1")
    with pytest.raises(_lib.BsigError, match="inflate"):
        Reads.from_bam(ctx, BamFile(str(p)))
    monkeypatch.setenv("BAMSIGNALS_DEVICE_DECODE", "require")
    with pytest.raises(_lib.BsigError, match="CPU decode path"):
        Reads.from_bam(ctx, BamFile(str(p)))
