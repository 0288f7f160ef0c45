/* video/rp_video.h — batched baseline-JPEG encoding of rendered frames (C ABI, gfx950, librp_video.so).
 *
 * One call turns `frame_count` RGB images, as rp_render writes them, into one complete JPEG file each (SOI to EOI):
 * the frames of a Motion-JPEG stream.  This comment DEFINES the bytes: every step is integer arithmetic, so an
 * implementation either gives these bytes or is wrong.  `>>` is the arithmetic (floor) shift, `/` integer division of
 * non-negative integers.
 *
 * Colour.  YCbCr 4:4:4 from 8-bit R, G, B:
 *     Y  =  (19595 R + 38470 G +  7471 B + 32768) >> 16
 *     Cb = ((-11059 R - 21709 G + 32768 B + 32768) >> 16) + 128
 *     Cr = (( 32768 R - 27439 G -  5329 B + 32768) >> 16) + 128
 * each clamped to [0, 255], then 128 is subtracted.
 *
 * Blocks.  The image is padded to Hp x Wp, multiples of 8, by repeating its last column and row, and cut into 8 x 8
 * tiles; X[r][c] is one component of one tile.
 *
 * DCT.  Ci[u][x] = rint(8192 c), c = sqrt(1/8) for u = 0 and 0.5 cos((2x+1) u pi / 16) otherwise (the 64 integers
 * are RPV_CI of csrc/rp_video.hpp).
 *     T[u][c] = (sum_r Ci[u][r] X[r][c] + 1024) >> 11
 *     F[u][v] = (sum_c T[u][c] Ci[v][c] + 16384) >> 15
 * Every intermediate fits in int32 (|.| <= 2^26).  The two passes are the definition; the implementation adds
 * x and 7 - x first (Ci[u][7-x] = (-1)^u Ci[u][x]), which gives the same integers.
 *
 * Quantisation.  q[u][v] = sign(F) ((|F| + Q/2) / Q).  Q is Annex K's luminance (Y) or chrominance (Cb, Cr) table
 * scaled by the IJG rule: s = 5000 / quality below 50, else 200 - 2 quality; Q = clamp((base s + 50) / 100, 1, 255).
 *
 * Entropy coding.  Baseline sequential Huffman with the four standard tables of Annex K (K.3 - K.6).  A block is
 * its coefficients in zigzag order: the DC difference to the previous block of the same component in the segment,
 * then (run, size) symbols.  A value v of size s (the bit length of |v|) is followed by s bits: v, or the low s bits
 * of v + 2^s - 1 when v < 0.  A run above 15 is written as ZRL (0xF0) symbols; EOB (0x00) ends a block unless
 * coefficient 63 is non-zero.
 *
 * Restart intervals.  The restart interval is one MCU row: Wp/8 MCUs, an MCU being the Y, Cb, Cr blocks of one
 * tile.  A SEGMENT is the entropy-coded data of one MCU row: its DC predictors start at 0, it is padded with 1-bits
 * to a whole byte, and every 0xFF byte in it, the pad byte included, is followed by 0x00.  Segment r < Hp/8 - 1 is
 * followed by the marker RSTm, m = r mod 8; the last one by EOI.  A segment depends on nothing outside its MCU row.
 *
 * File.  SOI; APP0 (JFIF 1.01, no units, density 1 x 1, no thumbnail); DQT 0 and DQT 1 (8 bit, zigzag order), one
 * segment each; SOF0 (8 bit, H, W, components 1 / 2 / 3, sampling 0x11, quantisation tables 0 / 1 / 1); four DHT
 * segments (DC 0, AC 0, DC 1, AC 1); DRI (Wp/8); SOS (components 1 / 2 / 3 with tables 0x00 / 0x11 / 0x11, 0, 63, 0);
 * the segments and their markers; EOI.  Everything before the first segment is the HEADER: it depends only on
 * (height, width, quality) and rp_video_header returns it.
 *
 * Size.  A block costs at most (11 + 11) + 63 (16 + 10) = 1660 bits (DC: code and value of 11 bits each; AC: code of
 * 16 and value of 10).  A segment of 3 Wp/8 blocks is therefore at most B = ceil(3 Wp/8 x 1660 / 8) bytes, pad bits
 * included; stuffing at most doubles them, and its marker adds 2:
 *     rp_video_max_bytes = header + (Hp/8) (2 B + 2)
 * (the last segment's "marker" is EOI).  With bytes_cap >= that, a frame always fits.
 *
 * Calls.  rgb, bytes and length are DEVICE pointers into caller-owned memory, rows indexed by the ABSOLUTE frame:
 * frames outside [frame_first, frame_first + frame_count) stay untouched.  length[f] is the file's size; a frame that
 * needs more than bytes_cap bytes gets the first bytes_cap bytes of its file, nothing past them, and
 * length[f] = -(bytes needed).  rp_video_encode only enqueues on `hip_stream` (hipStream_t; NULL = default stream):
 * no host synchronisation, no allocation after create; the handle's scratch (the quantised coefficients and the
 * segment sizes) is reused by every call, so calls on one handle must be ordered on the device.  Calls return 0, or a
 * negative code with the message in rp_video_last_error(); a refused call launches nothing.  No global atomics are
 * used: two runs give the same bytes.
 */
#ifndef RP_VIDEO_H_
#define RP_VIDEO_H_

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct rp_video rp_video;

typedef struct rp_video_encode_args {
  size_t struct_size;            /* sizeof(rp_video_encode_args) of the caller: a mismatch is refused */
  const unsigned char* rgb;      /* [N][H][W][3], N = max_frames */
  int frame_first, frame_count;  /* frames [frame_first, frame_first + frame_count) are encoded */
  int bytes_cap;                 /* bytes per row of `bytes`; >= 1 */
  unsigned char* bytes;          /* [N][bytes_cap] */
  int* length;                   /* [N] */
  void* hip_stream;
} rp_video_encode_args;

/* height, width in 1..65535, quality in 1..100.  Allocates the scratch of max_frames frames and uploads the tables. */
int rp_video_create(int height, int width, int max_frames, int quality, int device, rp_video** out);
void rp_video_destroy(rp_video* v);

int rp_video_encode(rp_video* v, const rp_video_encode_args* args);

/* The strict upper bound of one frame's bytes (above), or -1 for a NULL handle. */
int rp_video_max_bytes(const rp_video* v);

/* Copies the header to the HOST array `dst` (if not NULL; at most *n bytes) and sets *n to the header's size. */
int rp_video_header(const rp_video* v, unsigned char* dst, int* n);

/* "height", "width", "max_frames", "quality", "segments" (Hp/8), "segment_blocks" (3 Wp/8), "chunk_blocks" */
int rp_video_dim(const rp_video* v, const char* name);

const char* rp_video_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* RP_VIDEO_H_ */
