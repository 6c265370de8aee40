"""Generates tests/golden/containers_v1.json: the version-1 container formats of codec.py (LLDW, LLDT, LLDO, LLDR) pinned
byte for byte.  Host only, no GPU; the built library is needed for the LLDR table CRC alone (residual.tables).

    python tests/golden/make_containers.py

Every case is packed from seeded synthetic streams (random.Random(0)) and recorded as the length and sha256 of the container,
the header dict read_header gives back (digests as hex) and reduce_bytes of it.  ``cases()`` is what
tests/test_codec_golden_host.py repacks and reparses, so the inputs are defined once, here."""
import hashlib
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd import codec          # noqa: E402

OUT = os.path.join(HERE, "containers_v1.json")
L = 3
PER = 3 * (L + 1)
PLAIN = "cgp=f16x3,plc_algo=winograd,plc_fuse=1,plc_mode=f16x3,plc_shape=auto,precision=f16x3,storage=fp32"
ARITHMETICS = {"plain": PLAIN, "irans32": ",".join(sorted(PLAIN.split(",") + ["coder=irans32"])),
               "step23": codec._with_step(PLAIN, 23)}


def _streams(rng, n):
    """n streams of 0 .. 59 bytes; the second is empty and the third has 130 .. 299 bytes (a two-byte LEB128 length)."""
    lens = [rng.randrange(60) for _ in range(n)]
    lens[1], lens[2] = 0, rng.randrange(130, 300)
    return [bytes(rng.randrange(256) for _ in range(m)) for m in lens]


def _units(rng, n, near):
    return [dict(cs_xh=rng.getrandbits(64), cs_x=rng.getrandbits(64) if near == 0 else 0,
                 scales=bytes(rng.randrange(64) for _ in range(24)), streams=_streams(rng, 3)) for _ in range(n)]


def cases():
    """-> list of (name, pack, parse, args): pack(*args) is the container, parse(container) its parsed form."""
    from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd import residual
    rng = random.Random(0)
    out = []
    for key, arith in ARITHMETICS.items():
        hdr = dict(layer="conditioned2ZTsepSubbands", netType="LiftingBasedNeuralWaveletv4", dwtlevels=L, numerics=1,
                   arithmetic=arith, digest=bytes(rng.randrange(256) for _ in range(16)))
        lldw = (dict(hdr, H=37, W=53), _streams(rng, PER))
        lldt = (dict(hdr, H=100, W=150, th=40, tw=56, ny=3, nx=3), [_streams(rng, PER) for _ in range(9)])
        lldo = (dict(hdr, H=100, W=150, th=56, tw=56, ny=2, nx=3, overlap=8), [_streams(rng, PER) for _ in range(6)])
        out += [("lldw/" + key, codec.pack_container, codec.parse_container, lldw),
                ("lldt/" + key, codec.pack_tiled, codec.parse_tiled, lldt),
                ("lldo/" + key, codec.pack_lapped, codec.parse_lapped, lldo)]
        for base, pack, args, n in (("lldw", codec.pack_container, lldw, 1), ("lldt", codec.pack_tiled, lldt, 9)):
            for near in (0, 3):
                out.append(("lldr/%s/near%d/%s" % (base, near, key), codec.pack_refined, codec.parse_refined,
                            (near, residual.tables(near).crc, pack(*args), _units(rng, n, near))))
    return out


def jsonable(v):
    """A header dict with its digests (bytes, also in the nested base header of an LLDR) as hex."""
    if isinstance(v, dict):
        return {k: jsonable(x) for k, x in v.items()}
    return v.hex() if isinstance(v, bytes) else v


def record(blob):
    hdr = codec.read_header(blob)
    return dict(length=len(blob), sha256=hashlib.sha256(blob).hexdigest(), header=jsonable(hdr),
                reduce_bytes=codec.reduce_bytes(hdr))


def main():
    out = {name: record(pack(*args)) for name, pack, _, args in cases()}
    with open(OUT, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("ok", len(out), "cases")


if __name__ == "__main__":
    main()
