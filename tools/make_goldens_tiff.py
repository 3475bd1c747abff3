#!/opt/conda/bin/python3.9
"""Fixtures for the compressed-TIFF reader: small stacks written by tifffile (2021.7.2, with imagecodecs) in the layouts the
reader must open -- deflate strips, ragged last strip, BigTIFF, big-endian with the horizontal predictor, one strip per page,
ImageJ hyperstack page order, 8-bit -- an uncompressed twin, and one LZW file that must keep raising; and what the REFERENCE's
own `read_tiff` (bim.py:28-51) returns for each.

    /opt/conda/bin/python3.9 tools/make_goldens_tiff.py     -> tests/golden/tiff/*.tif, tests/golden/tiff/expected.npz

Every stack is seeded and of shape T2 x C2 x Z3 x 40 x 48 (46 KB raw).  Only data is written."""
import os
import sys
import types
import warnings

warnings.filterwarnings("ignore")
sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
REF = "/root/reference"
OUT = os.path.join(REPO, "tests", "golden", "tiff")


def _stub(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


_stub("aicsimageio", AICSImage=object)
_stub("aicsimageio.readers", czi_reader=None, bioformats_reader=None)
_stub("aicsimageio.writers", ome_tiff_writer=None)
sys.path.insert(0, os.path.join(REF, "tissue_analyzing_tool"))

import numpy as np  # noqa: E402
import tifffile  # noqa: E402
import basic_image_manipulations as ref_bim  # noqa: E402  (reference)


def stack(seed, dtype=np.uint16):
    """a smooth surface per plane plus noise: deflate finds both long matches and plain Huffman runs"""
    rng = np.random.default_rng(seed)
    t, c, z, yy, xx = np.meshgrid(np.arange(2), np.arange(2), np.arange(3), np.arange(40), np.arange(48), indexing="ij")
    top = 250 if dtype == np.uint8 else 60000
    a = top * (0.45 + 0.4 * np.sin((yy + 3 * z) / 6.0) * np.cos((xx + 5 * c + 2 * t) / 8.0)) + rng.integers(0, 9, yy.shape)
    a[:, :, :, 10:14, :] = 0                       # flat rows: long matches, and zeros under the predictor
    return a.astype(dtype)


def lzw_literals(data):
    """A TIFF LZW stream (codes most-significant bit first, ClearCode 256, EndOfInformation 257) that never uses the table: a
    ClearCode before every 250 bytes keeps every code at 9 bits.  (This imagecodecs build decodes LZW but has no encoder.)"""
    codes = []
    for i, b in enumerate(data):
        if i % 250 == 0:
            codes.append(256)
        codes.append(b)
    codes.append(257)
    bits = "".join(format(c, "09b") for c in codes)
    bits += "0" * (-len(bits) % 8)
    return bytes(int(bits[i:i + 8], 2) for i in range(0, len(bits), 8))


def write_lzw(path, data):
    """classic little-endian TIFF, one LZW strip per (Y, X) plane, tifffile's JSON description on the first page"""
    import json
    import struct
    planes = data.reshape((-1,) + data.shape[-2:]).astype("<u2")
    rows, cols = planes.shape[1:]
    desc = json.dumps({"shape": list(data.shape), "axes": "TCZYX"}).encode() + b"\0"
    desc += b"\0" * (len(desc) & 1)
    with open(path, "wb") as fh:
        fh.write(struct.pack("<2sHI", b"II", 42, 8))
        offset = 8
        for k, plane in enumerate(planes):
            strip = lzw_literals(plane.tobytes())
            strip += b"\0" * (len(strip) & 1)
            extra = desc if k == 0 else b""
            entries = [(256, 4, 1, cols), (257, 4, 1, rows), (258, 3, 1, 16), (259, 3, 1, 5), (262, 3, 1, 1), (277, 3, 1, 1),
                       (278, 4, 1, rows), (279, 4, 1, len(strip)), (339, 3, 1, 1)]
            ifd_size = 2 + 12 * (len(entries) + 1 + (1 if extra else 0)) + 4
            entries.append((273, 4, 1, offset + ifd_size + len(extra)))
            if extra:
                entries.append((270, 2, len(extra), offset + ifd_size))
            entries.sort()
            nxt = offset + ifd_size + len(extra) + len(strip) if k + 1 < len(planes) else 0
            fh.write(struct.pack("<H", len(entries)))
            for tag, typ, cnt, val in entries:
                fh.write(struct.pack("<HHII", tag, typ, cnt, val))
            fh.write(struct.pack("<I", nxt) + extra + strip)
            offset = nxt


def main():
    os.makedirs(OUT, exist_ok=True)
    base = stack(1)
    tcz = dict(metadata={"axes": "TCZYX"}, photometric="minisblack")     # (else tifffile takes Z = 3 for colour samples)
    files = [
        ("zlib_rps7", base, dict(compression="zlib", rowsperstrip=7, **tcz)),
        ("zlib_rps7_bigtiff", stack(2), dict(compression="zlib", rowsperstrip=7, bigtiff=True, **tcz)),
        ("zlib_predictor_bigendian", stack(3), dict(compression="zlib", predictor=True, rowsperstrip=7, byteorder=">", **tcz)),
        ("zlib_one_strip", stack(4), dict(compression="zlib", rowsperstrip=40, **tcz)),
        ("zlib_imagej", np.ascontiguousarray(stack(5).transpose(0, 2, 1, 3, 4)), dict(compression="zlib", rowsperstrip=7, imagej=True)),   # T Z C Y X
        ("zlib_u8", stack(6, np.uint8), dict(compression="zlib", rowsperstrip=7, **tcz)),
        ("plain_rps7", base, dict(rowsperstrip=7, **tcz)),
    ]
    expected = {}
    for name, data, kw in files + [("lzw", stack(7), None)]:
        path = os.path.join(OUT, name + ".tif")
        if kw is None:
            write_lzw(path, data)
        else:
            tifffile.imwrite(path, data, **kw)
        image, axes, shape, _ = ref_bim.read_tiff(path)
        assert np.array_equal(image, data) and tuple(shape) == data.shape, name
        with tifffile.TiffFile(path) as tif:
            page = tif.pages[0]
            print("%-26s %6d bytes  axes %-6s %s  compression %d predictor %d rowsperstrip %d strips/page %d %s%s" % (
                name, os.path.getsize(path), axes, image.dtype, page.compression, page.predictor, page.rowsperstrip,
                len(page.dataoffsets), tif.byteorder, " bigtiff" if tif.is_bigtiff else ""))
        expected[name + "__image"] = image
        expected[name + "__axes"] = np.array(axes)
        expected[name + "__shape"] = np.array(shape, np.int64)
    np.savez_compressed(os.path.join(OUT, "expected.npz"), **expected)


if __name__ == "__main__":
    main()
