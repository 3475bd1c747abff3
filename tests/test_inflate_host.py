"""CPU: the conditions on the case list of tests/inflate_cases.py, tip_inflate_strips_host (the decoder of
csrc/tip_inflate_core.h compiled for the host) on every case, and the sanitizer program tools/inflate_hostcheck.cpp, which
runs the same header under AddressSanitizer and UBSan over the cases and a few thousand mutations of them."""
import os
import shutil
import subprocess
import zlib

import numpy as np
import pytest

import inflate_cases as ic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the list itself ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c[0] for c in ic.VALID])
def test_zlib_inflates_every_valid_case(name):
    _, stream, wrapper, expected, dst_len, status = ic.BY_NAME[name]
    assert zlib.decompress(stream, 15 if wrapper else -15) == expected
    assert dst_len == len(expected) and status == "OK"


@pytest.mark.parametrize("name", [c[0] for c in ic.INVALID])
def test_zlib_rejects_every_invalid_case(name):
    _, stream, wrapper, expected, dst_len, status = ic.BY_NAME[name]
    assert expected is None and status != "OK"
    try:
        out = zlib.decompress(stream, 15 if wrapper else -15)
    except zlib.error:
        return
    assert len(out) != dst_len


def test_valid_cases_cover_the_format():
    """All three block types, a code of 15 bits, and both wrappers -- found by walking the streams with the tests' own inflate."""
    types, longest = set(), 0
    for name, stream, wrapper, expected, _, _ in ic.VALID:
        out, t, l = ic.walk(stream, wrapper)
        assert out == expected, name
        types |= t
        longest = max(longest, l)
        if name.startswith("stored"):
            assert t == {0}, name
        if name.startswith("fixed"):
            assert t == {1}, name
        if name.startswith(("dynamic", "codes_15_bits", "literals_only")):
            assert 2 in t, name
        if name.startswith("three_parts"):
            assert 0 in t, name              # the flush markers: empty stored blocks
    assert types == {0, 1, 2}
    assert longest == 15
    assert ic.walk(ic.BY_NAME["codes_15_bits_raw"][1], 0)[2] == 15
    assert {c[2] for c in ic.VALID} == {0, 1}
    assert len(ic.INVALID) == 14 and len({c[5] for c in ic.INVALID}) == 10       # every status word but OK


def test_hand_made_tokens_are_what_they_claim():
    """distance_1: a literal, a match of 258 and one of 3, all at distance 1 (what zlib's Z_RLE writes for 262 equal bytes)."""
    stream = ic.BY_NAME["distance_1_raw"][1]
    w = ic.BitWriter().value(1, 1).value(1, 2)
    ic.fixed_lit(w, ord("a"))
    ic.fixed_match(w, 258, 1)
    ic.fixed_match(w, 3, 1)
    for ch in b"tail":
        ic.fixed_lit(w, ch)
    ic.fixed_lit(w, 256)
    assert w.bytes() == stream


# ---- the host decoder ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wrapper", [0, 1])
def test_host_decoder_on_every_case(wrapper):
    """Packed several to a call, guards before, between and after: zlib's bytes and status 0 on the valid cases, the named status on
    the invalid ones, every guard byte intact."""
    from tissue_image_processing_amd import _inflate
    cases = [c for c in ic.CASES if c[2] == wrapper]
    src, strips, dst = ic.pack(cases)
    status, n_bad = _inflate.inflate_strips_host(src, strips, wrapper, dst)
    ic.check_packed(cases, strips, dst, status, _inflate.STATUS)
    assert n_bad == sum(c[5] != "OK" for c in cases)


def test_host_decoder_checks_the_table():
    from tissue_image_processing_amd import _inflate
    name, stream, _, data, n, _ = ic.BY_NAME["fixed_raw"]
    src = np.frombuffer(stream, np.uint8)

    def call(rows, dst_bytes=2 * n + 8):
        dst = np.zeros(dst_bytes, np.uint8)
        out = _inflate.inflate_strips_host(src, np.array(rows, np.int64).reshape(-1, 4), 0, dst)
        return out, dst

    (status, n_bad), dst = call([(0, src.size, 0, n), (0, src.size, n, n)])      # the same source twice is fine
    assert n_bad == 0 and dst[:n].tobytes() == data and dst[n:2 * n].tobytes() == data
    for rows in ([(0, src.size, 0, n), (0, src.size, n - 1, n)],                   # destinations overlap by one byte
                 [(0, src.size, 4, n), (0, src.size, 0, 5)],
                 [(1, src.size, 0, n)], [(0, src.size + 1, 0, n)], [(-1, 4, 0, n)], [(0, -1, 0, n)],      # source out of range
                 [(0, src.size, n + 9, n)], [(0, src.size, -1, n)], [(0, src.size, 0, 2 * n + 9)], [(0, src.size, 0, -1)],
                 [(2 ** 62, 2 ** 62, 0, n)], [(0, src.size, 2 ** 62, 2 ** 62)]):
        with pytest.raises(ValueError):
            call(rows)
    (status, n_bad), dst = call([(0, src.size, 8, 0), (0, src.size, 0, n)])      # an empty destination inside another overlaps nothing
    assert n_bad == 1 and status[0] == _inflate.STATUS["OUTPUT_FULL"] and dst[:n].tobytes() == data
    with pytest.raises(ValueError):
        _inflate.inflate_strips_host(src, np.array([(0, src.size, 0, n)], np.int64), 2, np.zeros(n, np.uint8))
    status, n_bad = _inflate.inflate_strips_host(src, np.zeros((0, 4), np.int64), 0, np.zeros(4, np.uint8))
    assert status.size == 0 and n_bad == 0


# ---- the same header under the sanitizers ---------------------------------------------------------------------------------------
def test_sanitizer_program(tmp_path):
    """tools/inflate_hostcheck.cpp: a stand-alone program, built for the host with -fsanitize=address,undefined and run directly.
    It decodes every case from exactly-sized source buffers into guarded destinations, then 6000 fixed-seed single-byte and
    truncation mutations of the valid streams: any status, a clean return, intact guards."""
    # the sanitizer runtimes are linked into the program (g++ needs the flags, clang does it by default): it runs as it is, in
    # whatever environment the suite runs in
    exe, cases = str(tmp_path / "inflate_hostcheck"), str(tmp_path / "cases.bin")
    tried = []
    for cxx, extra in ((os.environ.get("CXX"), []), ("g++", ["-static-libasan", "-static-libubsan"]), ("clang++", []),
                       ("/opt/rocm/llvm/bin/clang++", [])):
        if not cxx or not shutil.which(cxx):
            continue
        build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + extra +
                               ["-I", os.path.join(ROOT, "tissue_image_processing_amd", "csrc"),
                                os.path.join(ROOT, "tools", "inflate_hostcheck.cpp"), "-o", exe],
                               stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        if build.returncode == 0:
            break
        tried.append("%s: %s" % (cxx, build.stdout[-500:]))
    else:
        pytest.fail("no host C++ compiler built the sanitizer program:\n" + "\n".join(tried))
    ic.dump(cases)
    run = subprocess.run([exe, cases], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(run.stdout)
    assert run.returncode == 0, run.stdout[-4000:]
    assert "cases %d ok" % len(ic.CASES) in run.stdout and "mutations 6000 ok" in run.stdout
