"""Host (CPU) tests of 9- to 16-bit coding: the depth key of the arithmetic string, the LLDW / LLDT containers
that carry it, the argument pairs and tensor types the encoders refuse, the wrapper containers over a keyed base, and the PPM /
PGM reader and writer of tools/codec.py.  Nothing here touches the GPU."""
import importlib.util
import os
import struct
import zlib

import numpy as np
import pytest
import torch

from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd import codec

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASE = "cgp=f16,plc_algo=direct,plc_fuse=1,plc_mode=f16x3,plc_shape=16,precision=f16x3,storage=fp32"
DIGEST = bytes(range(16))
L = 3


def _hdr(arith, H=64, W=96):
    return dict(layer="onlyEZWT", netType="LiftingBasedNeuralWaveletv4", dwtlevels=L, H=H, W=W,
                numerics=codec.CODING_NUMERICS_VERSION, arithmetic=arith, digest=DIGEST)


def _streams(count, seed=0):
    return [bytes((seed + 7 * i + j) & 0xFF for j in range(3 + i)) for i in range(count)]


def _reseal(body):
    return bytes(body) + struct.pack("<I", zlib.crc32(bytes(body)) & 0xFFFFFFFF)


def _rekey(blob, old, new):
    """The container with its arithmetic string ``old`` replaced by ``new`` and the CRC redone."""
    at = blob.index(old.encode())
    return _reseal(blob[:at - 1] + bytes([len(new)]) + new.encode() + blob[at + len(old):-4])


def _tool():
    spec = importlib.util.spec_from_file_location("codec_cli_depth", os.path.join(REPO, "tools", "codec.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    return cli


# ------------------------------------------------------------------------------------------------ the arithmetic string
def test_the_depth_key_round_trips_and_8_bits_have_none():
    assert codec._with_depth(BASE, None) == BASE and codec._with_depth(BASE, 8) == BASE
    assert codec._split_depth(BASE) == (8, BASE)
    assert codec.check_depth(None) == 8 and codec.check_depth(8) == 8
    for d in range(9, 17):
        a = codec._with_depth(BASE, d)
        assert "depth=%d" % d in a.split(",") and a.split(",") == sorted(a.split(","))
        assert codec._split_depth(a) == (d, BASE) and codec.check_depth(d) == d
    # its sorted place beside coder, step and chroma, in any order of merging: chroma < coder < depth < plc_algo, step last
    full = codec._with_depth(codec._with_chroma(codec._with_step(BASE + ",coder=irans32", 40), "420"), 12)
    keys = [p.split("=")[0] for p in full.split(",")]
    assert keys == sorted(keys) and keys[:5] == ["cgp", "chroma", "coder", "depth", "plc_algo"] and keys[-1] == "storage"
    assert codec._split_depth(full) == (12, codec._with_chroma(codec._with_step(BASE + ",coder=irans32", 40), "420"))
    rest = codec._split_depth(full)[1]
    assert codec._split_chroma(rest)[0] == "420" and codec._split_step(codec._split_chroma(rest)[1])[0] == 40
    assert codec._split_chroma(full)[0] == "420" and codec._split_step(full)[0] == 40 and codec._split_coder(full)[0] == "gpu"
    assert codec._batch_invariant(full) == codec._batch_invariant(BASE)
    for bad in (7, 17, 0, -1, 12.0, "12", True):
        with pytest.raises(ValueError, match="depth"):
            codec.check_depth(bad)


def test_arithmetic_string_takes_the_depth(monkeypatch):
    from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd import ops
    for name, val in (("cgp_mode", "f16"), ("plc_algo", "direct"), ("plc_fuse", True), ("plc_mode", "f16x3"), ("plc_shape", "16"),
                      ("get_precision", "f16x3"), ("storage_dtype", "fp32")):
        monkeypatch.setattr(ops, name, lambda v=val: v)
    assert codec.arithmetic_string() == BASE == codec.arithmetic_string(depth=None) == codec.arithmetic_string(depth=8)
    a = codec.arithmetic_string("gpu", 2.5, chroma="420", depth=10)
    assert codec._split_depth(a) == (10, codec.arithmetic_string("gpu", 2.5, chroma="420"))
    with pytest.raises(ValueError, match="depth"):
        codec.arithmetic_string(depth=17)


MALFORMED = ["depth=8", "depth=17", "depth=012", "depth=1e1", "depth=12,depth=12", "depth=", "depth=+12", "depth= 12"]


@pytest.mark.parametrize("bad", MALFORMED)
def test_a_malformed_depth_key_is_refused_by_every_reader(bad):
    with pytest.raises(ValueError, match="depth"):
        codec._split_depth(BASE + "," + bad)
    arith = ",".join(sorted(BASE.split(",") + bad.split(",")))
    blob = _rekey(codec.pack_container(_hdr(BASE), _streams(12)), BASE, arith)
    tiled = _rekey(codec.pack_tiled(dict(_hdr(BASE, H=100, W=64), th=64, tw=64, ny=2, nx=1), [_streams(12, 1), _streams(12, 2)]),
                   BASE, arith)
    with pytest.raises(ValueError, match="depth"):
        codec.parse_container(blob)
    with pytest.raises(ValueError, match="depth"):
        codec.parse_tiled(tiled)
    for b in (blob, tiled):
        with pytest.raises(ValueError, match="depth"):
            codec.read_header(b)


# ------------------------------------------------------------------------------------------------ the containers
@pytest.mark.parametrize("ch,planes", [("444", 3), ("420", 3), ("400", 1)])
def test_lldw_and_lldt_round_trip_with_the_key(ch, planes):
    arith = codec._with_depth(codec._with_chroma(BASE, ch), 12)
    streams = _streams(planes * (L + 1))
    blob = codec.pack_container(_hdr(arith), streams)
    hdr, got = codec.parse_container(blob)
    assert got == streams and hdr["depth"] == 12 and hdr["arithmetic"] == arith and hdr.get("chroma", "444") == ch
    assert codec.read_header(blob) == hdr and blob[:4] == b"LLDW" and blob[4] == codec.FORMAT_VERSION
    assert codec.reduce_bytes(hdr)[0] == len(blob) - 4
    tiles = [_streams(planes * (L + 1), seed=1), _streams(planes * (L + 1), seed=2)]
    tb = codec.pack_tiled(dict(_hdr(arith, H=100, W=96), th=64, tw=96, ny=2, nx=1), tiles)
    thdr, tgot = codec.parse_tiled(tb)
    assert tgot == tiles and thdr["depth"] == 12 and tb[:4] == b"LLDT" and tb[4] == codec.TILED_FORMAT_VERSION
    # the identity check sets the key aside, like coder, step and chroma
    codec.check_header(hdr, "onlyEZWT", "LiftingBasedNeuralWaveletv4", L, DIGEST, BASE)
    with pytest.raises(ValueError, match="arithmetic"):
        codec.check_header(hdr, "onlyEZWT", "LiftingBasedNeuralWaveletv4", L, DIGEST, BASE.replace("direct", "winograd"))


def test_a_key_less_container_is_8_bits_and_gains_no_entry():
    blob = codec.pack_container(_hdr(BASE), _streams(12))
    hdr, _ = codec.parse_container(blob)
    assert "depth" not in hdr and hdr.get("depth", 8) == 8 and "depth" not in hdr["arithmetic"]
    assert blob == codec.pack_container(_hdr(codec._with_depth(BASE, 8)), _streams(12))


def test_wrappers_and_lapped_tiles_refuse_a_base_with_the_key():
    from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd import quality_layers as ql
    plain = codec._with_step(BASE, 48)
    arith = codec._with_depth(plain, 10)
    base = codec.pack_container(_hdr(arith), _streams(3 * (L + 1)))
    with pytest.raises(ValueError, match="depth.*layers"):
        codec.pack_layered(ql.tables().crc, base, [[[b"x"] * (3 * (L - 1))]])
    with pytest.raises(ValueError, match="depth.*near"):
        codec.pack_refined(0, 0, base, [dict(cs_xh=0, cs_x=0, scales=bytes(24), streams=[b""] * 3)])
    with pytest.raises(ValueError, match="depth.*step_map"):
        codec.pack_mapped(np.full((8, 12), 16, dtype=np.int64), base)
    lapped = dict(_hdr(arith, H=100, W=64), th=64, tw=64, ny=2, nx=1, overlap=16)
    with pytest.raises(ValueError, match="depth.*overlap"):
        codec.pack_lapped(lapped, [_streams(12)] * 2)
    # and the parsers: wrappers packed over an 8-bit base whose arithmetic string is given the key afterwards
    lo = codec.pack_lapped(dict(lapped, arithmetic=plain), [_streams(12, 1), _streams(12, 2)])
    with pytest.raises(ValueError, match="depth.*overlap"):
        codec.read_header(_rekey(lo, plain, arith))
    base8 = codec.pack_container(_hdr(plain), _streams(12))
    keyed = _rekey(base8, plain, arith)
    assert len(keyed) == len(base8) + len(",depth=10")
    lay = codec.pack_layered(ql.tables().crc, base8, [[[b"x"] * (3 * (L - 1))]])
    ref = codec.pack_refined(0, 0, base8, [dict(cs_xh=0, cs_x=0, scales=bytes(24), streams=[b""] * 3)])
    for wrapper, parse, name in ((lay, lambda b: codec.parse_layered(b, check_tables=False), "layers"),
                                 (ref, lambda b: codec.parse_refined(b, check_tables=False), "near")):
        old = codec.leb128_encode(len(base8)) + base8                               # the base with its length before it
        at = wrapper.index(old)
        bad = _reseal(wrapper[:at] + codec.leb128_encode(len(keyed)) + keyed + wrapper[at + len(old):-4])
        with pytest.raises(ValueError, match="depth.*%s" % name):
            parse(bad)
        with pytest.raises(ValueError, match="depth.*%s" % name):
            codec.read_header(bad)


# ------------------------------------------------------------------------------------------------ refusals
PAIRS = (("near", dict(near=0)), ("near", dict(near=2)), ("layers", dict(layers=1)), ("step_map", dict(step_map=[[1.0]])),
         ("overlap", dict(overlap=16)), ("target_psnr", dict(target_psnr=30.0)), ("target_msssim", dict(target_msssim=0.9)))


def test_refused_argument_pairs_raise_on_the_host():
    args = codec._depth_args
    assert args(None) == 8 and args(8, near=0, layers=2, overlap=16, target_psnr=30.0, step_map=[[1.0]]) == 8
    assert args(12) == 12 and args(16, layers=0) == 16 and args(9, layers=None, overlap=0) == 9
    for d in (9, 12, 16):
        for name, kw in PAIRS:
            with pytest.raises(ValueError, match="depth and %s" % name):
                args(d, **kw)
    for bad in (7, 17, "12"):
        with pytest.raises(ValueError, match="depth"):
            args(bad)


def test_check_images_knows_the_depth():
    u8, u16 = torch.zeros(1, 4, 5, 3, dtype=torch.uint8), torch.zeros(1, 4, 5, 3, dtype=torch.uint16)
    assert codec._check_images(u8) == (1, 4, 5) == codec._check_images(u16, depth=12)
    assert codec._check_images(torch.zeros(2, 4, 5, 1, dtype=torch.uint16), "400", 16) == (2, 4, 5)
    with pytest.raises(ValueError, match="depth"):
        codec._check_images(u16)                                       # uint16 without a depth
    with pytest.raises(ValueError, match="depth"):
        codec._check_images(u8, depth=12)                              # uint8 with one
    with pytest.raises(ValueError, match=r"\(B,H,W,1\) uint16"):
        codec._check_images(u16, "400", 12)
    with pytest.raises(ValueError, match="uint16"):
        codec._check_images(torch.zeros(1, 4, 5, 3, dtype=torch.int16), depth=12)


def test_the_encoders_refuse_on_the_host_before_any_gpu_work(monkeypatch):
    """Through the public entry points, with the library unreachable: every refusal of the list and the tensor type rules."""
    from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd import _lib
    from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd.graphs.models.LiftingBasedDWT_net import \
        LiftingBasedDWTNetWrapper
    from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd.utils.config import make_config
    net = LiftingBasedDWTNetWrapper(make_config(dwtlevels=3, mode="validate")).eval()

    def no_library():
        raise AssertionError("the GPU library was loaded")
    monkeypatch.setattr(_lib, "load", no_library)
    u8, u16 = torch.zeros(1, 24, 40, 3, dtype=torch.uint8), torch.zeros(1, 24, 40, 3, dtype=torch.uint16)
    for enc in (codec.encode_images, codec.encode_tiled):
        for name, kw in (("near", dict(near=0)), ("layers", dict(layers=1, step=3.0)), ("step_map", dict(step_map=[[1.0] * 5] * 3)),
                         ("target_psnr", dict(target_psnr=30.0)), ("target_msssim", dict(target_msssim=0.9))):
            with pytest.raises(ValueError, match="depth and %s" % name):
                enc(net, u16, depth=12, **kw)
        with pytest.raises(ValueError, match="depth"):
            enc(net, u16)
        with pytest.raises(ValueError, match="depth"):
            enc(net, u16, depth=8)
        with pytest.raises(ValueError, match="depth"):
            enc(net, u8, depth=12)
        with pytest.raises(ValueError, match="depth"):
            enc(net, u16, depth=17)
    with pytest.raises(ValueError, match="depth and overlap"):
        codec.encode_tiled(net, u16, depth=12, overlap=16)
    for a, b, kw in ((u16, u16, {}), (u8, u8, dict(depth=12)), (u16, u16, dict(depth=7))):
        with pytest.raises(ValueError, match="depth"):
            codec.quality(a, b, **kw)


def test_decode_images_refuses_a_mix_of_depths(monkeypatch):
    from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd.graphs.models.LiftingBasedDWT_net import \
        LiftingBasedDWTNetWrapper
    from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd.utils.config import make_config
    net = LiftingBasedDWTNetWrapper(make_config(dwtlevels=3, mode="validate")).eval()
    blobs = [codec.pack_container(_hdr(codec._with_depth(BASE, d)), _streams(12)) for d in (None, 12)]
    with pytest.raises(ValueError, match="depth"):
        codec.decode_images(net, blobs)


# ------------------------------------------------------------------------------------------------ the tool's PPM / PGM files
def test_pnm_reader_and_writer_round_trip(tmp_path):
    cli = _tool()
    g = np.random.default_rng(0)
    for d in (8, 10, 16):
        M = (1 << d) - 1
        rgb = g.integers(0, M + 1, (5, 7, 3)).astype(np.uint16)
        rgb[0, 0] = (M, 0, 1)
        grey = rgb[..., 1].copy()
        for name, a in (("a.ppm", rgb), ("a.pgm", grey)):
            path = str(tmp_path / ("%d_%s" % (d, name)))
            cli.write_pnm(path, a, M)
            raw = open(path, "rb").read()
            head = b"%s\n7 5\n%d\n" % (b"P6" if a.ndim == 3 else b"P5", M)
            assert raw.startswith(head) and len(raw) == len(head) + a.size * (2 if d > 8 else 1)
            if d > 8:                                                  # big-endian 16-bit samples, per Netpbm
                assert raw[len(head):len(head) + 4] == struct.pack(">HH", int(a.reshape(-1)[0]), int(a.reshape(-1)[1]))
            back, maxval = cli.read_pnm(path)
            assert maxval == M and back.shape == a.shape and np.array_equal(back, a)
            assert back.dtype == (np.uint16 if d > 8 else np.uint8)
    # comments and any whitespace between the header's tokens
    path = str(tmp_path / "c.pgm")
    with open(path, "wb") as f:
        f.write(b"P5 # a comment\n# another\n2\t1\n1023\n" + struct.pack(">HH", 1023, 513))
    back, maxval = cli.read_pnm(path)
    assert maxval == 1023 and back.tolist() == [[1023, 513]]
    x = cli.load_deep(path, 10, grey=True)
    assert x.dtype == torch.uint16 and tuple(x.shape) == (1, 2, 1)
    with pytest.raises(ValueError, match="maxval"):
        cli.load_deep(path, 12, grey=True)
    with pytest.raises(ValueError, match="RGB"):
        cli.load_deep(path, 10)
    with open(path, "wb") as f:
        f.write(b"P5\n2 1\n1023\n\x00")
    with pytest.raises(ValueError, match="sample bytes"):
        cli.read_pnm(path)
    with open(path, "wb") as f:
        f.write(b"P3\n2 1\n255\n1 2")
    with pytest.raises(ValueError, match="binary"):
        cli.read_pnm(path)
    # .npy goes through as it is; the extension chooses the writer
    np.save(str(tmp_path / "x.npy"), rgb)
    assert torch.equal(cli.load_deep(str(tmp_path / "x.npy"), 16), torch.from_numpy(rgb))
    cli.save_deep(str(tmp_path / "y.npy"), torch.from_numpy(rgb), 16)
    assert np.array_equal(np.load(str(tmp_path / "y.npy")), rgb)
    cli.save_deep(str(tmp_path / "y.ppm"), torch.from_numpy(rgb), 16)
    assert np.array_equal(cli.read_pnm(str(tmp_path / "y.ppm"))[0], rgb)
    with pytest.raises(ValueError, match="ppm"):
        cli.save_deep(str(tmp_path / "y.png"), torch.from_numpy(rgb), 16)
