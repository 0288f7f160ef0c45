"""Reference for the JPEG encoder's tests: a numpy restatement of the byte stream's definition
(include/video/rp_video.h), the shared test cases, and the g++ build of csrc/rp_video.hpp.

The restatement takes nothing from the C++ text.  Its DCT integers come from the formula, and its quantisation and
Huffman tables are read out of a file that the local Pillow (libjpeg) writes: a non-optimised JPEG of quality 50 carries
Annex K's tables K.1 - K.6 as they stand.  The stream is defined in integers, so every comparison is byte equality.
"""

from __future__ import annotations

import ctypes
import functools
import io
import math
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- tables ----------------------------------------------------------------------------------------------------------
def zigzag():
    """natural index 8 u + v of zigzag position z"""
    order = []
    for s in range(15):
        cells = [(i, s - i) for i in range(8) if 0 <= s - i < 8]
        order += [8 * r + c for r, c in (cells[::-1] if s % 2 == 0 else cells)]
    return np.array(order)


def dct_integers():
    """Ci[u][x] = rint(8192 c(u, x))"""
    ci = np.zeros((8, 8), np.int64)
    for u in range(8):
        for x in range(8):
            c = math.sqrt(1.0 / 8.0) if u == 0 else 0.5 * math.cos((2 * x + 1) * u * math.pi / 16.0)
            ci[u, x] = int(np.rint(8192.0 * c))
    return ci


def parse_segments(data: bytes):
    """[(marker, payload)] of a JPEG file's header, up to and including SOS; and the offset of the entropy-coded data."""
    assert data[:2] == b"\xff\xd8"
    out, i = [], 2
    while True:
        assert data[i] == 0xFF, f"no marker at {i}"
        marker, n = data[i + 1], data[i + 2] * 256 + data[i + 3]
        out.append((marker, data[i + 4:i + 2 + n]))
        i += 2 + n
        if marker == 0xDA:
            return out, i


def parse_dht(payload: bytes):
    """{class byte: (bits[16], vals)} of one DHT payload (which may hold several tables)"""
    tables, j = {}, 0
    while j < len(payload):
        bits = list(payload[j + 1:j + 17])
        n = sum(bits)
        tables[payload[j]] = (bits, list(payload[j + 17:j + 17 + n]))
        j += 17 + n
    return tables


def parse_tables(data: bytes):
    """(dqt {id: 64 zigzag values}, dht {class: (bits, vals)}) of a JPEG file"""
    dqt, dht = {}, {}
    for marker, payload in parse_segments(data)[0]:
        if marker == 0xDB:
            for j in range(0, len(payload), 65):
                assert payload[j] >> 4 == 0
                dqt[payload[j] & 15] = list(payload[j + 1:j + 65])
        elif marker == 0xC4:
            dht.update(parse_dht(payload))
    return dqt, dht


def pillow_jpeg(rgb, **kwargs) -> bytes:
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(rgb, np.uint8)).save(buf, "JPEG", **kwargs)
    return buf.getvalue()


@functools.lru_cache(maxsize=None)
def annex_k():
    """(base quantisation tables {0, 1: zigzag}, Huffman tables {class: (bits, vals)}) out of a libjpeg file of quality
    50 (scale factor 100: the base tables themselves)"""
    dqt, dht = parse_tables(pillow_jpeg(np.zeros((8, 8, 3), np.uint8), quality=50, subsampling=0))
    assert sorted(dqt) == [0, 1] and sorted(dht) == [0x00, 0x01, 0x10, 0x11]
    return dqt, dht


def quant_tables(quality: int):
    """[luminance, chrominance] in zigzag order by the IJG rule"""
    s = 5000 // quality if quality < 50 else 200 - 2 * quality
    base = annex_k()[0]
    return [np.clip((np.array(base[t], np.int64) * s + 50) // 100, 1, 255) for t in (0, 1)]


def huffman_codes(bits, vals):
    """{symbol: (code, length)}: codes of each length counted up, shifted left at each new length"""
    codes, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            codes[vals[k]] = (code, length)
            code, k = code + 1, k + 1
        code <<= 1
    return codes


def header(height, width, quality) -> bytes:
    q = quant_tables(quality)
    dht = annex_k()[1]
    nbx = (width + 7) // 8
    h = b"\xff\xd8" + b"\xff\xe0\x00\x10JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00"
    for t in (0, 1):
        h += b"\xff\xdb\x00\x43" + bytes([t]) + bytes(int(x) for x in q[t])
    h += b"\xff\xc0\x00\x11\x08" + height.to_bytes(2, "big") + width.to_bytes(2, "big") + b"\x03\x01\x11\x00\x02\x11\x01\x03\x11\x01"
    for cls in (0x00, 0x10, 0x01, 0x11):
        bits, vals = dht[cls]
        h += b"\xff\xc4" + (19 + len(vals)).to_bytes(2, "big") + bytes([cls]) + bytes(bits) + bytes(vals)
    h += b"\xff\xdd\x00\x04" + nbx.to_bytes(2, "big")
    h += b"\xff\xda\x00\x0c\x03\x01\x00\x02\x11\x03\x11\x00\x3f\x00"
    return h


def max_bytes(height, width, quality=90):
    nbx, nby = (width + 7) // 8, (height + 7) // 8
    per_segment = (3 * nbx * 1660 + 7) // 8
    return len(header(height, width, quality)) + nby * (2 * per_segment + 2)


# ---- the definition --------------------------------------------------------------------------------------------------
def coefficients(rgb, quality):
    """Quantised coefficients [nby][nbx][3][64] in zigzag order, int64."""
    rgb = np.asarray(rgb)
    H, W = rgb.shape[:2]
    R, G, B = (rgb[..., i].astype(np.int64) for i in range(3))
    Y = (19595 * R + 38470 * G + 7471 * B + 32768) >> 16
    Cb = ((-11059 * R - 21709 * G + 32768 * B + 32768) >> 16) + 128
    Cr = ((32768 * R - 27439 * G - 5329 * B + 32768) >> 16) + 128
    ycc = np.clip(np.stack([Y, Cb, Cr]), 0, 255) - 128
    Hp, Wp = (H + 7) // 8 * 8, (W + 7) // 8 * 8
    ycc = np.pad(ycc, ((0, 0), (0, Hp - H), (0, Wp - W)), mode="edge")
    X = ycc.reshape(3, Hp // 8, 8, Wp // 8, 8).transpose(1, 3, 0, 2, 4)          # [ty][tx][comp][r][c]
    ci = dct_integers()
    T = (np.einsum("ur,...rc->...uc", ci, X) + 1024) >> 11
    F = (np.einsum("...uc,vc->...uv", T, ci) + 16384) >> 15
    assert np.abs(T).max() < 2 ** 26 and np.abs(F).max() < 2 ** 26
    F = F.reshape(F.shape[:3] + (64,))[..., zigzag()]
    q = quant_tables(quality)
    Q = np.stack([q[0], q[1], q[1]])
    return np.sign(F) * ((np.abs(F) + Q // 2) // Q)


def _size(v):
    return int(abs(int(v))).bit_length()


def _value_bits(v, s):
    return (v if v >= 0 else v + (1 << s) - 1) & ((1 << s) - 1)


CHUNK_BLOCKS = 64   # blocks the device codes side by side (rp_video_dim "chunk_blocks"; the host test compares the two)


def _chunk_stats(st, data, ends, start, chunk_blocks):
    """What one segment adds to the chunk counters of `stats`.  `data` are the segment's bytes before stuffing (padded),
    `ends` the bit count after each of its blocks, `start` the file offset of data[0].  Chunk j holds blocks
    [j chunk_blocks, (j + 1) chunk_blocks); its whole bytes are data[lo:hi], with lo where the previous chunk's whole
    bytes ended and hi = (bits up to its end) // 8; the bits behind them are carried.  The last chunk takes the pad."""
    raw = np.frombuffer(data, np.uint8)
    is_ff = raw == 0xFF
    at = start + np.arange(len(raw)) + np.concatenate([[0], np.cumsum(is_ff)[:-1]])   # file offset of each data byte
    st["stuffed_at"] += [int(x) + 1 for x in at[is_ff]]
    st["max_block_bits"] = max(st["max_block_bits"], int(np.diff([0] + ends).max()))
    edges = [ends[min(k + chunk_blocks, len(ends)) - 1] for k in range(0, len(ends), chunk_blocks)]
    edges[-1] = 8 * len(raw)
    st["chunks"] = max(st["chunks"], len(edges))
    lo = 0
    for j, end in enumerate(edges):
        hi = end // 8
        # what the chunk's bit buffer holds: the carried bits, the chunk's own and (last chunk) the pad
        st["max_chunk_bits"] = max(st["max_chunk_bits"], end - 8 * lo)
        st["group_edge_ff"] += int(is_ff[lo + 63:hi:64].sum())
        st["group_edge_at"] += [int(x) for x in at[lo + 63:hi:64][is_ff[lo + 63:hi:64]]]
        if j < len(edges) - 1:
            assert hi > lo
            if end % 8 == 0:
                st["seam_aligned"] += 1
            else:
                st["seam_at"].append(int(at[hi]))
                st["seam_ff"] += bool(is_ff[hi])
            st["seam_prev_ff"] += bool(is_ff[hi - 1])
            if is_ff[hi - 1]:
                st["seam_prev_at"].append(int(at[hi - 1]) + 1)
        lo = hi


def encode(rgb, quality, stats=None, chunk_blocks=CHUNK_BLOCKS) -> bytes:
    """The JPEG file of one image.  `stats` (a dict) collects what the symbol stream contains: counts of the symbols
    and, from the symbol stream alone, of what falls on the seams between chunks of `chunk_blocks` blocks:
      seam_ff        bytes that hold bits of two chunks and equal 0xFF
      seam_aligned   chunks (but the last of a segment) that end on a byte boundary
      seam_prev_ff   chunks (but the last) whose last whole byte is 0xFF
      group_edge_ff  0xFF bytes at index 63 mod 64 among one chunk's whole bytes
      max_block_bits, max_chunk_bits (the carried bits and the pad included), chunks (per segment), segments
    and where things are in the file: seg_at (the first byte of each segment, then the file's length; segment s's
    marker is the two bytes before seg_at[s + 1]), stuffed_at (the stuffed zeros), seam_at (the bytes that hold bits of
    two chunks), seam_prev_at (the stuffed zeros of seam_prev_ff), group_edge_at (the 0xFF bytes of group_edge_ff)."""
    rgb = np.asarray(rgb)
    H, W = rgb.shape[:2]
    coef = coefficients(rgb, quality)
    nby, nbx = coef.shape[:2]
    dht = annex_k()[1]
    dc = [huffman_codes(*dht[0x00]), huffman_codes(*dht[0x01])]
    ac = [huffman_codes(*dht[0x10]), huffman_codes(*dht[0x11])]
    st = stats if stats is not None else {}
    for k in ("zrl", "no_eob", "neg_dc", "neg_ac", "stuffed", "stuffed_pad", "seam_ff", "seam_aligned", "seam_prev_ff",
              "group_edge_ff", "max_block_bits", "max_chunk_bits", "chunks"):
        st.setdefault(k, 0)
    for k in ("seg_at", "stuffed_at", "seam_at", "seam_prev_at", "group_edge_at"):
        st.setdefault(k, [])
    st["max_dc_size"] = st.get("max_dc_size", 0)
    st["max_ac_size"] = st.get("max_ac_size", 0)
    st["segments"], st["segment_blocks"] = nby, 3 * nbx
    out = bytearray(header(H, W, quality))
    for ty in range(nby):
        acc, nbits = 0, 0
        pred = [0, 0, 0]
        ends = []
        st["seg_at"].append(len(out))
        for tx in range(nbx):
            for c in range(3):
                t = 1 if c else 0
                blk = coef[ty, tx, c]
                d = int(blk[0]) - pred[c]
                pred[c] = int(blk[0])
                s = _size(d)
                st["max_dc_size"] = max(st["max_dc_size"], s)
                st["neg_dc"] += d < 0
                code, n = dc[t][s]
                acc, nbits = (((acc << n) | code) << s) | _value_bits(d, s), nbits + n + s
                last = 0
                for z in np.flatnonzero(blk[1:]) + 1:
                    z, v = int(z), int(blk[z])
                    run = z - last - 1
                    while run > 15:
                        code, n = ac[t][0xF0]
                        acc, nbits, run = (acc << n) | code, nbits + n, run - 16
                        st["zrl"] += 1
                    s = _size(v)
                    st["max_ac_size"] = max(st["max_ac_size"], s)
                    st["neg_ac"] += v < 0
                    code, n = ac[t][(run << 4) | s]
                    acc, nbits = (((acc << n) | code) << s) | _value_bits(v, s), nbits + n + s
                    last = z
                if last != 63:
                    code, n = ac[t][0x00]
                    acc, nbits = (acc << n) | code, nbits + n
                else:
                    st["no_eob"] += 1
                ends.append(nbits)
        pad = -nbits % 8
        acc, nbits = (acc << pad) | ((1 << pad) - 1), nbits + pad
        data = acc.to_bytes(nbits // 8, "big")
        st["stuffed"] += data.count(b"\xff")
        st["stuffed_pad"] += bool(pad) and data[-1] == 0xFF
        _chunk_stats(st, data, ends, len(out), chunk_blocks)
        out += data.replace(b"\xff", b"\xff\x00")
        out += b"\xff" + bytes([0xD9 if ty == nby - 1 else 0xD0 + ty % 8])
    st["seg_at"].append(len(out))
    return bytes(out)


# ---- cases -----------------------------------------------------------------------------------------------------------
def gradient(H, W):
    """Three different ramps, with a saturated rectangle (pure red: Cr clamps) in the middle."""
    y, x = np.mgrid[0:H, 0:W]
    img = np.stack([(x * 255) // max(W - 1, 1), (y * 255) // max(H - 1, 1), ((x + y) * 255) // max(H + W - 2, 1)], -1)
    img[H // 4:H // 2 + 1, W // 4:W // 2 + 1] = (255, 0, 0)
    return img.astype(np.uint8)


def noise(H, W, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (H, W, 3), dtype=np.uint8)


def pixel_checkerboard(H, W):
    y, x = np.mgrid[0:H, 0:W]
    return np.repeat((((x + y) & 1) * 255).astype(np.uint8)[..., None], 3, -1)


def block_checkerboard(H, W):
    y, x = np.mgrid[0:H, 0:W]
    return np.repeat(((((x // 8) + (y // 8)) & 1) * 255).astype(np.uint8)[..., None], 3, -1)


def sign_pattern(H, W):
    """Every tile is black and white by the sign of the (4,4) basis function: the largest AC coefficient there is."""
    ci = dct_integers()
    tile = np.where(np.outer(ci[4], ci[4]) > 0, 255, 0).astype(np.uint8)
    img = np.tile(tile, ((H + 7) // 8, (W + 7) // 8))[:H, :W]
    return np.repeat(img[..., None], 3, -1)


def flat(H, W):
    """One colour.  (216, 44, 22) is one of the colours that the 8-bit YCbCr round trip returns exactly (about one in four
    does; that is the colour transform's rounding, whoever encodes), so at quality 100 the image decodes exactly."""
    return np.full((H, W, 3), (216, 44, 22), np.uint8)


def rendered_like(H, W):
    """Large flat regions with sharp edges, as the ray caster draws them: a shaded floor, a row of white and black keys,
    two skin-coloured slabs at an angle, a background band."""
    y, x = np.mgrid[0:H, 0:W]
    img = np.zeros((H, W, 3), np.int64)
    img[:] = (77, 102, 128)
    floor = y > H // 3
    img[floor] = np.stack([60 + (y * 40) // max(H, 1)] * 3, -1)[floor]
    keys = (y > H // 2) & (y < (3 * H) // 4)
    img[keys & ((x * 26 // max(W, 1)) % 2 == 0)] = (235, 235, 235)
    img[keys & ((x * 26 // max(W, 1)) % 2 == 1)] = (20, 20, 20)
    for x0, slope in ((W // 5, 2), ((3 * W) // 5, -3)):
        slab = (np.abs((x - x0) * 4 - (y - H // 2) * slope) < max(W // 6, 2)) & (y > H // 4) & (y < (2 * H) // 3)
        img[slab] = (214, 160, 120)
    return img.astype(np.uint8)


CONTENTS = dict(gradient=gradient, noise=noise, pixel_checkerboard=pixel_checkerboard,
                block_checkerboard=block_checkerboard, sign_pattern=sign_pattern, flat=flat, rendered_like=rendered_like)

# 80 x 176: 66 blocks per segment (one more chunk of 2), 10 segments (the RST counter wraps); 72 x 168: 63 blocks, one
# short of a chunk (3 blocks per tile: 64 is no multiple); 8 x 344: 129 blocks, three chunks, bits carried twice
SIZES = ((8, 8), (1, 1), (9, 17), (30, 44), (84, 84), (80, 176), (72, 168), (8, 344))

PAD_STUFF_CASE = ("noise", (8, 8), 100, 15)   # found by search_pad_stuff_seed(): its only segment ends in a 0xFF pad byte


def search_pad_stuff_seed(limit=200):
    """The first seed whose 8 x 8 noise at quality 100 ends in a stuffed pad byte (how PAD_STUFF_CASE was found)."""
    for seed in range(limit):
        st = {}
        encode(noise(8, 8, seed), 100, st)
        if st["stuffed_pad"]:
            return seed
    return None


def saturated(H, W, seed=0):
    """Noise whose every channel is 0 or 255: the most pixel energy there is, hence the longest codes."""
    return (np.random.default_rng(seed).integers(0, 2, (H, W, 3), dtype=np.uint8) * 255).astype(np.uint8)


SEEDED = dict(noise=noise, saturated=saturated)


def search_seam_seed(event, size, quality, limit, first=0):
    """The first seed in [first, limit) whose noise of `size` at `quality` shows `event` (one of the chunk counters of
    encode's stats) at least once, or None: how the SEAM_*_CASEs below were found."""
    for seed in range(first, limit):
        st = {}
        encode(noise(size[0], size[1], seed), quality, st)
        if st[event]:
            return seed
    return None


# ---- the wide cases: what the wave-level bookkeeping of the device's packing can get wrong ---------------------------
# More than 64 segments (the layout scans them 64 at a time and carries the sum): 520 x 8 is one more than a round;
# 1025 x 1 three rounds with padding below and to the right; 513 x 17 65 segments of 9 blocks, padded both ways.
TALL_CASES = (("noise", (520, 8), 90, 0), ("noise", (520, 8), 100, 0), ("noise", (1025, 1), 90, 0),
              ("noise", (513, 17), 90, 0))
# 387 blocks: seven chunks, bits carried six times; 24 rows: three such segments in one frame.
MANY_CHUNK_CASES = (("noise", (8, 1032), 100, 0), ("rendered_like", (8, 1032), 90, 0),
                    ("noise", (24, 1032), 100, 0), ("rendered_like", (24, 1032), 90, 0))
# Found by search_seam_seed(event, (8, 344), 100, 2000), the first seed each; the count is the event's in that case.
SEAM_FF_CASE = ("noise", (8, 344), 100, 4)        # seam_ff 1: the byte that chunk 1's bits complete is 0xFF
SEAM_ALIGNED_CASE = ("noise", (8, 344), 100, 3)   # seam_aligned 1: a chunk ends on a byte boundary, nothing is carried
# seam_prev_ff 1 (and seam_aligned 2): a chunk whose last whole byte is 0xFF.  Quality 100 has none: seeds 0..1999 of
# 8 x 344 and of 80 x 176 (24,000 seams) show no such chunk.  search_seam_seed("seam_prev_ff", (80, 176), 98, 600).
SEAM_PREV_FF_CASE = ("noise", (80, 176), 98, 9)
# Every channel 0 or 255. Reaches max_block_bits 881 and max_chunk_bits 51,218 at 8 x 176, 900 and 51,383 at 8 x 344
# (the buffer is sized for 1660 and 106,240; the fullest chunk of the cases before these held 44,897 bits).
DENSE_CASES = (("saturated", (8, 176), 100, 0), ("saturated", (8, 344), 100, 0))


@functools.lru_cache(maxsize=None)
def base_case_list():
    """((content, (H, W), quality, seed), ...): every size with noise at 90 and the gradient at 50; every content at
    every quality at 30 x 44; the extremes (quality 100 noise: every coefficient is there, so no EOB, long segments and
    0xFF bytes; the checkerboard of blocks: DC differences of size 11; the sign pattern: AC values of size 10) on the
    sizes that cross a chunk; the rendered-like image at the sizes of a camera observation."""
    cases = []
    for size in SIZES:
        cases += [("noise", size, 90, 0), ("gradient", size, 50, 0)]
    for content in CONTENTS:
        for quality in (1, 50, 90, 100):
            cases.append((content, (30, 44), quality, 0))
    for size in ((80, 176), (72, 168), (8, 344)):
        cases += [("noise", size, 100, 1), ("block_checkerboard", size, 100, 0), ("rendered_like", size, 90, 0)]
    cases += [("sign_pattern", (8, 8), 100, 0), ("flat", (8, 8), 100, 0), ("flat", (1, 1), 1, 0),
              ("rendered_like", (84, 84), 90, 0), ("rendered_like", (84, 84), 50, 0), ("rendered_like", (80, 176), 50, 0),
              ("sign_pattern", (80, 176), 100, 0), ("block_checkerboard", (84, 84), 100, 0), PAD_STUFF_CASE]
    return tuple(dict.fromkeys(cases))


@functools.lru_cache(maxsize=None)
def case_list():
    """base_case_list(), then the wide cases: tall frames, many chunks, the seam events, the dense chunks."""
    wide = TALL_CASES + MANY_CHUNK_CASES + (SEAM_FF_CASE, SEAM_ALIGNED_CASE, SEAM_PREV_FF_CASE) + DENSE_CASES
    return tuple(dict.fromkeys(base_case_list() + wide))


def case_id(case):
    content, (H, W), quality, seed = case
    return f"{content}-{H}x{W}-q{quality}" + (f"-s{seed}" if seed else "")


def case_image(case):
    content, (H, W), quality, seed = case
    img = SEEDED[content](H, W, seed) if content in SEEDED else CONTENTS[content](H, W)
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def case_reference(case):
    """(the restatement's file, its stats) of one case; computed once."""
    st = {}
    data = encode(case_image(case), case[2], st)
    return data, st


def groups():
    """{(H, W, quality): [cases]}: the cases one encoder can take as one batch."""
    out = {}
    for case in case_list():
        out.setdefault((case[1][0], case[1][1], case[2]), []).append(case)
    return out


def psnr(a, b):
    mse = np.mean((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2)
    return float("inf") if mse == 0 else 10.0 * math.log10(255.0 ** 2 / mse)


def decode(data: bytes):
    from PIL import Image
    im = Image.open(io.BytesIO(data))
    im.load()
    return im


FIDELITY_CASES = tuple(c for c in (
    [(content, (30, 44), q, 0) for content in CONTENTS for q in (50, 90)] +
    [("rendered_like", (84, 84), 90, 0), ("rendered_like", (84, 84), 50, 0), ("rendered_like", (80, 176), 90, 0),
     ("rendered_like", (80, 176), 50, 0)]))


def measure_fidelity(encoder):
    """Per fidelity case: PSNR (dB) of libjpeg's own encoding with our tables minus the PSNR of encoder(image, quality),
    both decoded by Pillow, against the source: the deficit, positive where we are worse.  Returns {case id: deficit}."""
    out = {}
    for case in FIDELITY_CASES:
        img = case_image(case)
        q = quant_tables(case[2])
        # (Pillow takes qtables in natural order; the file stores them in zigzag order, which the assertion checks)
        natural = [[int(t[z]) for z in np.argsort(zigzag())] for t in q]
        theirs = pillow_jpeg(img, qtables=natural, subsampling=0)
        assert parse_tables(theirs)[0] == {0: [int(x) for x in q[0]], 1: [int(x) for x in q[1]]}
        p_theirs = psnr(np.asarray(decode(theirs).convert("RGB")), img)
        p_ours = psnr(np.asarray(decode(encoder(img, case[2])).convert("RGB")), img)
        out[case_id(case)] = 0.0 if p_theirs == p_ours else p_theirs - p_ours
    return out


# ---- the g++ build of csrc/rp_video.hpp ------------------------------------------------------------------------------
_HOST_SRC = r"""
#include "rp_video.hpp"
struct rp_video { RpvTables tab; int max_frames; };
static thread_local std::string g_err;
static int fail(const std::string& s) { g_err = s; return -1; }
extern "C" {
const char* rpvh_last_error(void) { return g_err.c_str(); }
int rpvh_create(int height, int width, int max_frames, int quality, int device, rp_video** out) {
  (void)device;
  rp_video* v = new rp_video();
  const std::string err = v->tab.build(height, width, max_frames, quality);
  if (!err.empty()) { delete v; return fail("rp_video_create: " + err); }
  v->max_frames = max_frames;
  *out = v;
  return 0;
}
void rpvh_destroy(rp_video* v) { delete v; }
int rpvh_encode(rp_video* v, const rp_video_encode_args* g) {
  const std::string err = rpv_check_args(g, v->max_frames);
  if (!err.empty()) return fail(err);
  rpv_encode_host(v->tab, g);
  return 0;
}
int rpvh_max_bytes(const rp_video* v) { return (int)v->tab.max_bytes; }
int rpvh_header(const rp_video* v, unsigned char* dst, int* n) {
  const int have = (int)v->tab.header.size();
  if (dst) memcpy(dst, v->tab.header.data(), (size_t)(*n < have ? *n : have));
  *n = have;
  return 0;
}
int rpvh_dim(const rp_video* v, const char* name) {
  return !strcmp(name, "segments") ? v->tab.G.nby : !strcmp(name, "segment_blocks") ? v->tab.G.seg_blocks : !strcmp(name, "chunk_blocks") ? RPV_CHUNK : -1;
}
const int* rpvh_dct_integers(void) { return RPV_CI; }
const int* rpvh_zigzag(void) { return RPV_ZIGZAG; }
/* n / Q by rpv_div against the division itself, over every n < 2^16 and Q in 1..255: the number of mismatches */
int rpvh_div_mismatches(void) {
  int bad = 0;
  for (unsigned Q = 1; Q <= 255; Q++) {
    const uint32_t m = (uint32_t)((1ull << 31) / Q + 1);
    for (unsigned n = 0; n < 65536; n++) bad += rpv_div(n, m) != n / Q;
  }
  return bad;
}
}
"""

# A program of its own for the sanitizers: the extreme cases through the host routines, every output buffer exactly as
# long as the file (a write past it is a heap overflow), the cap one short of it once more.
_SANITIZER_MAIN = r"""
#include <stdio.h>
#include <stdlib.h>
#include "rp_video.hpp"
static int run(int H, int W, int quality, int kind) {
  RpvTables tab;
  const std::string err = tab.build(H, W, 1, quality);
  if (!err.empty()) { printf("build: %s\n", err.c_str()); return 1; }
  unsigned char* rgb = (unsigned char*)malloc((size_t)H * W * 3);
  unsigned s = 12345u + (unsigned)kind;
  for (int y = 0; y < H; y++)
    for (int x = 0; x < W; x++)
      for (int c = 0; c < 3; c++) {
        s = s * 1664525u + 1013904223u;
        const int checker = ((x / 8 + y / 8) & 1) * 255;
        rgb[((size_t)y * W + x) * 3 + c] = (unsigned char)(kind == 0 ? (s >> 24) : kind == 1 ? checker : 77);
      }
  std::vector<unsigned char> file;
  rpv_encode_frame_host(tab, rgb, file);
  if ((long long)file.size() > tab.max_bytes) { printf("%zu bytes exceed the bound %lld\n", file.size(), tab.max_bytes); return 1; }
  int rc = 0;
  for (int shave = 0; shave < 2 && !rc; shave++) {
    const int cap = (int)file.size() - shave;
    unsigned char* out = (unsigned char*)malloc((size_t)cap);
    int length = 0;
    rp_video_encode_args a;
    memset(&a, 0, sizeof(a));
    a.struct_size = sizeof(a); a.rgb = rgb; a.frame_first = 0; a.frame_count = 1; a.bytes_cap = cap; a.bytes = out; a.length = &length;
    if (!rpv_check_args(&a, 1).empty()) rc = 1;
    rpv_encode_host(tab, &a);
    if (length != (shave ? -(int)file.size() : (int)file.size()) || memcmp(out, file.data(), (size_t)cap)) rc = 1;
    free(out);
  }
  free(rgb);
  printf("%dx%d q%d kind %d: %zu bytes%s\n", H, W, quality, kind, file.size(), rc ? " FAILED" : "");
  return rc;
}
int main() {
  int rc = 0;
  const int sizes[][2] = {{1, 1}, {8, 8}, {9, 17}, {80, 176}, {8, 344}};
  for (auto& hw : sizes)
    for (int kind = 0; kind < 3; kind++) {
      rc |= run(hw[0], hw[1], 100, kind);
      rc |= run(hw[0], hw[1], 1, kind);
    }
  return rc;
}
"""

_host_lib = None
_host_dir = None


def _csrc():
    return os.path.join(ROOT, "robopianist_amd", "csrc")


def host_library():
    """Compiles csrc/rp_video.hpp with g++ (once per process) and loads the result."""
    global _host_lib, _host_dir
    if _host_lib is None:
        from robopianist_amd import video
        _host_dir = tempfile.TemporaryDirectory(prefix="rp_video_host_")
        src = os.path.join(_host_dir.name, "rp_video_host.cpp")
        so = os.path.join(_host_dir.name, "librp_video_host.so")
        with open(src, "w") as fh:
            fh.write(_HOST_SRC)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I", _csrc(), src, "-o", so])
        L = ctypes.CDLL(so)
        video.declare(L, "rpvh_")
        L.rpvh_dct_integers.restype = ctypes.POINTER(ctypes.c_int)
        L.rpvh_zigzag.restype = ctypes.POINTER(ctypes.c_int)
        _host_lib = L
    return _host_lib


def build_sanitizer_program(directory):
    """Compiles the stand-alone program with AddressSanitizer and UBSan, their runtimes linked statically (the program
    then runs the same whatever else the process loads first); returns (path or None, the compiler's output)."""
    src = os.path.join(directory, "rp_video_sanitize.cpp")
    exe = os.path.join(directory, "rp_video_sanitize")
    with open(src, "w") as fh:
        fh.write(_SANITIZER_MAIN)
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-static-libasan", "-static-libubsan",
                        "-I", _csrc(), src, "-o", exe], capture_output=True, text=True)
    return (exe if r.returncode == 0 else None), r.stdout + r.stderr


class HostVideo:
    """The library's calls on the CPU (rpv_encode_host), numpy arrays in and out."""

    def __init__(self, height, width, max_frames=1, quality=90):
        from robopianist_amd import video
        self._V = video
        self._L = host_library()
        self.height, self.width, self.max_frames, self.quality = height, width, max_frames, quality
        self._h = ctypes.c_void_p()
        if self._L.rpvh_create(height, width, max_frames, quality, 0, ctypes.byref(self._h)) != 0:
            raise RuntimeError(self._L.rpvh_last_error().decode())
        self.max_bytes = self._L.rpvh_max_bytes(self._h)
        self.header = video.read_header(self._L, self._h, "rpvh_")

    def __del__(self):
        try:
            if self._h:
                self._L.rpvh_destroy(self._h)
        except Exception:
            pass

    def encode_into(self, rgb, out, length, frame_first=0, frame_count=None, struct_size=None):
        """rpvh_encode into the caller's arrays; returns the C return code."""
        rgb = np.ascontiguousarray(rgb, np.uint8)
        assert rgb.shape == (self.max_frames, self.height, self.width, 3)
        a = self._V.make_args(frame_first, self.max_frames - frame_first if frame_count is None else frame_count,
                              out.shape[1], rgb=rgb.ctypes.data, out_bytes=out.ctypes.data, length=length.ctypes.data)
        if struct_size is not None:
            a.struct_size = struct_size
        return self._L.rpvh_encode(self._h, ctypes.byref(a))

    def last_error(self):
        return self._L.rpvh_last_error().decode()

    def frames(self, rgb, bytes_cap=None):
        out = np.zeros((self.max_frames, self.max_bytes if bytes_cap is None else bytes_cap), np.uint8)
        length = np.zeros(self.max_frames, np.int32)
        if self.encode_into(rgb, out, length) != 0:
            raise RuntimeError(self.last_error())
        return [out[f, :max(int(length[f]), 0)].tobytes() for f in range(self.max_frames)], length
