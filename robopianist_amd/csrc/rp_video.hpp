// rp_video.hpp -- the JPEG encoder's routines (include/video/rp_video.h has the definition of the byte stream).
//
// Plain C++ behind RPV_HD, free of wave intrinsics: rp_video.hip compiles it for gfx950, and the CPU tests compile the
// same text with g++ (tests/video_reference.py), where rpv_encode_host walks frames, segments and blocks in order.
//
// What is shared: the tables, the per-block routines (rpv_load_block: colour and padding; rpv_transform_block: DCT and
// quantisation, coefficients out in zigzag order; rpv_walk: the symbols of one block into a bit sink) and the header.
// What is not: how the bits of a segment's blocks are packed side by side.  The kernels do it with a wave prefix sum
// and LDS atomic-or, the host with one sequential bit writer; both feed the same rpv_walk.
#pragma once

#include <stdint.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../include/video/rp_video.h"

#if defined(__HIPCC__)
#define RPV_HD __host__ __device__
#else
#define RPV_HD
#endif
#define RPV_INLINE RPV_HD inline __attribute__((always_inline))

#define RPV_CHUNK 64                        /* blocks of a segment coded side by side: one per lane */
#define RPV_BLOCK_BITS 1660                 /* (11 + 11) + 63 (16 + 10) */
#define RPV_MAX_DIM 65535

// Ci[u][x] = rint(8192 c(u, x)) (rp_video.h); tests recompute it
static constexpr int RPV_CI[64] = {
    2896,  2896,  2896,  2896,  2896,  2896,  2896,  2896,
    4017,  3406,  2276,   799,  -799, -2276, -3406, -4017,
    3784,  1567, -1567, -3784, -3784, -1567,  1567,  3784,
    3406,  -799, -4017, -2276,  2276,  4017,   799, -3406,
    2896, -2896, -2896,  2896,  2896, -2896, -2896,  2896,
    2276, -4017,   799,  3406, -3406,  -799,  4017, -2276,
    1567, -3784,  3784, -1567, -1567,  3784, -3784,  1567,
     799, -2276,  3406, -4017,  4017, -3406,  2276,  -799,
};

// natural index (8 u + v) of zigzag position z
static constexpr int RPV_ZIGZAG[64] = {
    0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28,
    35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63,
};

// Annex K tables K.1 (luminance) and K.2 (chrominance), natural order
static constexpr int RPV_BASE_Q[2][64] = {
    {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,  14, 13, 16, 24, 40,  57,  69,  56,  14, 17, 22, 29, 51,  87,  80,  62,
     18, 22, 37, 56, 68,  109, 103, 77,  24, 35, 55, 64, 81,  104, 113, 92,  49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99},
    {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99},
};

// Annex K tables K.3 - K.6 as DHT segments carry them: codes per length 1..16, then the symbols.  Order: DC 0, AC 0,
// DC 1, AC 1 (tests compare them with the DHT segments of a file written by libjpeg)
static constexpr unsigned char RPV_DHT_CLASS[4] = {0x00, 0x10, 0x01, 0x11};
static constexpr unsigned char RPV_DHT_BITS[4][16] = {
    {0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0},
    {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125},
    {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0},
    {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119},
};
static constexpr int RPV_DHT_COUNT[4] = {12, 162, 12, 162};
static constexpr unsigned char RPV_DHT_VALS[4][162] = {
    {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11},
    {1,   2,   3,   0,   4,   17,  5,   18,  33,  49,  65,  6,   19,  81,  97,  7,   34,  113, 20,  50,  129, 145, 161, 8,   35,  66,  177,
     193, 21,  82,  209, 240, 36,  51,  98,  114, 130, 9,   10,  22,  23,  24,  25,  26,  37,  38,  39,  40,  41,  42,  52,  53,  54,  55,
     56,  57,  58,  67,  68,  69,  70,  71,  72,  73,  74,  83,  84,  85,  86,  87,  88,  89,  90,  99,  100, 101, 102, 103, 104, 105, 106,
     115, 116, 117, 118, 119, 120, 121, 122, 131, 132, 133, 134, 135, 136, 137, 138, 146, 147, 148, 149, 150, 151, 152, 153, 154, 162, 163,
     164, 165, 166, 167, 168, 169, 170, 178, 179, 180, 181, 182, 183, 184, 185, 186, 194, 195, 196, 197, 198, 199, 200, 201, 202, 210, 211,
     212, 213, 214, 215, 216, 217, 218, 225, 226, 227, 228, 229, 230, 231, 232, 233, 234, 241, 242, 243, 244, 245, 246, 247, 248, 249, 250},
    {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11},
    {0,   1,   2,   3,   17,  4,   5,   33,  49,  6,   18,  65,  81,  7,   97,  113, 19,  34,  50,  129, 8,   20,  66,  145, 161, 177, 193,
     9,   35,  51,  82,  240, 21,  98,  114, 209, 10,  22,  36,  52,  225, 37,  241, 23,  24,  25,  26,  38,  39,  40,  41,  42,  53,  54,
     55,  56,  57,  58,  67,  68,  69,  70,  71,  72,  73,  74,  83,  84,  85,  86,  87,  88,  89,  90,  99,  100, 101, 102, 103, 104, 105,
     106, 115, 116, 117, 118, 119, 120, 121, 122, 130, 131, 132, 133, 134, 135, 136, 137, 138, 146, 147, 148, 149, 150, 151, 152, 153, 154,
     162, 163, 164, 165, 166, 167, 168, 169, 170, 178, 179, 180, 181, 182, 183, 184, 185, 186, 194, 195, 196, 197, 198, 199, 200, 201, 202,
     210, 211, 212, 213, 214, 215, 216, 217, 218, 226, 227, 228, 229, 230, 231, 232, 233, 234, 242, 243, 244, 245, 246, 247, 248, 249, 250},
};

// ---- tables of one (height, width, quality) -------------------------------------------------------------------------
// Division by Q as a multiplication: for n < 2^16 and 1 <= Q <= 255, n / Q == (2 n m) >> 32 with m = 2^31 / Q + 1
// (m Q = 2^31 + e with 0 < e <= Q, so the quotient is off by n e / (2^31 Q) < 2^-7 / Q: never enough to reach the next
// integer).  |F| + Q/2 stays below 2^12.  Zigzag order, as the kernels use them.
struct RpvQuant {     // by value into the transform kernel
  uint32_t half[2][64];
  uint32_t recip[2][64];
};

struct RpvHuff {      // code | length << 16, indexed by the symbol; 0 where the table has no code
  uint32_t dc[2][12];
  uint32_t ac[2][256];
};

RPV_INLINE uint32_t rpv_div(uint32_t n, uint32_t recip) { return (uint32_t)(((uint64_t)(2u * n) * recip) >> 32); }

struct RpvGeom {      // by value into the kernels
  int H, W;
  int nbx, nby;       // tiles per row, tile rows (= segments)
  int seg_blocks;     // 3 nbx
  int header_bytes;
};

struct RpvTables {
  int quality = 0;
  RpvGeom G{};
  unsigned char q[2][64];   // zigzag order, as DQT carries them
  RpvQuant quant;
  RpvHuff huff;
  std::vector<unsigned char> header;
  long long max_bytes = 0;

  static std::string check(int height, int width, int max_frames, int quality) {
    if (height < 1 || height > RPV_MAX_DIM || width < 1 || width > RPV_MAX_DIM) return "height and width must be in 1..65535";
    if (quality < 1 || quality > 100) return "quality must be in 1..100";
    if (max_frames < 1) return "max_frames must be positive";
    const long long nbx = (width + 7) / 8, nby = (height + 7) / 8;
    if ((long long)max_frames * nby * nbx * 3 > 0x7fff0000ll) return "max_frames x blocks per frame must stay below 2^31";
    return "";
  }

  std::string build(int height, int width, int max_frames, int quality_) {
    const std::string err = check(height, width, max_frames, quality_);
    if (!err.empty()) return err;
    quality = quality_;
    G.H = height; G.W = width; G.nbx = (width + 7) / 8; G.nby = (height + 7) / 8; G.seg_blocks = 3 * G.nbx;
    const int s = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    for (int t = 0; t < 2; t++)
      for (int z = 0; z < 64; z++) {
        int Q = (RPV_BASE_Q[t][RPV_ZIGZAG[z]] * s + 50) / 100;
        Q = Q < 1 ? 1 : (Q > 255 ? 255 : Q);
        q[t][z] = (unsigned char)Q;
        quant.half[t][z] = (uint32_t)(Q / 2);
        quant.recip[t][z] = (uint32_t)((1ull << 31) / (unsigned)Q + 1);
      }
    memset(&huff, 0, sizeof(huff));
    for (int t = 0; t < 4; t++) {
      uint32_t code = 0;
      int k = 0;
      for (int len = 1; len <= 16; len++) {
        for (int i = 0; i < RPV_DHT_BITS[t][len - 1]; i++, k++, code++) {
          const int sym = RPV_DHT_VALS[t][k];
          uint32_t* tab = (t & 1) ? huff.ac[t >> 1] : huff.dc[t >> 1];
          tab[sym] = code | ((uint32_t)len << 16);
        }
        code <<= 1;
      }
    }
    header.clear();
    auto put = [&](std::initializer_list<int> b) { for (int x : b) header.push_back((unsigned char)x); };
    put({0xFF, 0xD8});
    put({0xFF, 0xE0, 0, 16, 'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0});
    for (int t = 0; t < 2; t++) {
      put({0xFF, 0xDB, 0, 67, t});
      for (int z = 0; z < 64; z++) header.push_back(q[t][z]);
    }
    put({0xFF, 0xC0, 0, 17, 8, height >> 8, height & 255, width >> 8, width & 255, 3, 1, 0x11, 0, 2, 0x11, 1, 3, 0x11, 1});
    for (int t = 0; t < 4; t++) {
      const int n = RPV_DHT_COUNT[t];
      put({0xFF, 0xC4, (n + 19) >> 8, (n + 19) & 255, RPV_DHT_CLASS[t]});
      for (int i = 0; i < 16; i++) header.push_back(RPV_DHT_BITS[t][i]);
      for (int i = 0; i < n; i++) header.push_back(RPV_DHT_VALS[t][i]);
    }
    put({0xFF, 0xDD, 0, 4, G.nbx >> 8, G.nbx & 255});
    put({0xFF, 0xDA, 0, 12, 3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0});
    G.header_bytes = (int)header.size();
    const long long B = ((long long)G.seg_blocks * RPV_BLOCK_BITS + 7) / 8;
    max_bytes = G.header_bytes + (long long)G.nby * (2 * B + 2);
    if (max_bytes > 0x7fffffffll) return "a frame of this size may need more than 2^31 - 1 bytes";
    return "";
  }
};

inline std::string rpv_check_args(const rp_video_encode_args* g, int max_frames) {
  if (!g) return "rp_video_encode: args is NULL";
  if (g->struct_size != sizeof(rp_video_encode_args)) return "rp_video_encode: struct_size does not match this library";
  if (g->frame_first < 0 || g->frame_count < 1 || (long long)g->frame_first + g->frame_count > max_frames)
    return "rp_video_encode: frame window out of range";
  if (g->bytes_cap < 1) return "rp_video_encode: bytes_cap must be positive";
  if (!g->rgb || !g->bytes || !g->length) return "rp_video_encode: rgb, bytes and length must not be NULL";
  return "";
}

// ---- one block ------------------------------------------------------------------------------------------------------
// X[8 r + c] of component comp (0 Y, 1 Cb, 2 Cr) of tile (ty, tx) of one frame `rgb` [H][W][3]
RPV_INLINE void rpv_load_block(const unsigned char* __restrict__ rgb, int H, int W, int ty, int tx, int comp, int* X) {
  const int k0 = comp == 0 ? 19595 : (comp == 1 ? -11059 : 32768);
  const int k1 = comp == 0 ? 38470 : (comp == 1 ? -21709 : -27439);
  const int k2 = comp == 0 ? 7471 : (comp == 1 ? 32768 : -5329);
  const int off = comp == 0 ? 0 : 128;
#pragma unroll
  for (int r = 0; r < 8; r++) {
    const int y = ty * 8 + r < H ? ty * 8 + r : H - 1;
    const unsigned char* row = rgb + (size_t)y * W * 3;
#pragma unroll
    for (int c = 0; c < 8; c++) {
      const int x = tx * 8 + c < W ? tx * 8 + c : W - 1;
      const unsigned char* p = row + (size_t)x * 3;
      int v = ((k0 * (int)p[0] + k1 * (int)p[1] + k2 * (int)p[2] + 32768) >> 16) + off;
      v = v < 0 ? 0 : (v > 255 ? 255 : v);
      X[8 * r + c] = v - 128;
    }
  }
}

// out[u] = (sum_x Ci[u][x] in[x * stride] + round) >> shift, x and 7 - x added first
template <int ROUND, int SHIFT>
RPV_INLINE void rpv_dct8(const int* in, int in_stride, int* out, int out_stride) {
  int s[4], d[4];
#pragma unroll
  for (int j = 0; j < 4; j++) {
    s[j] = in[j * in_stride] + in[(7 - j) * in_stride];
    d[j] = in[j * in_stride] - in[(7 - j) * in_stride];
  }
#pragma unroll
  for (int u = 0; u < 8; u++) {
    const int* a = (u & 1) ? d : s;
    const int acc = RPV_CI[8 * u] * a[0] + RPV_CI[8 * u + 1] * a[1] + RPV_CI[8 * u + 2] * a[2] + RPV_CI[8 * u + 3] * a[3];
    out[u * out_stride] = (acc + ROUND) >> SHIFT;
  }
}

// quantised coefficients of X in zigzag order, two per word (even z in the low half): zz[32]
RPV_INLINE void rpv_transform_block(const int* X, const uint32_t* __restrict__ half, const uint32_t* __restrict__ recip, uint32_t* zz) {
  int T[64], F[64];
#pragma unroll
  for (int c = 0; c < 8; c++) rpv_dct8<1024, 11>(X + c, 8, T + c, 8);          // T[u][c], down the columns
#pragma unroll
  for (int u = 0; u < 8; u++) rpv_dct8<16384, 15>(T + 8 * u, 1, F + 8 * u, 1);  // F[u][v], along the rows
#pragma unroll
  for (int z = 0; z < 64; z++) {
    const int f = F[RPV_ZIGZAG[z]];
    const uint32_t a = (uint32_t)(f < 0 ? -f : f);
    const int qv = (int)rpv_div(a + half[z], recip[z]);
    const uint32_t h = (uint32_t)(f < 0 ? -qv : qv) & 0xffffu;
    if (z & 1) zz[z >> 1] |= h << 16; else zz[z >> 1] = h;
  }
}

RPV_INLINE int rpv_coef(const uint32_t* zz, int z) { return (int)(int16_t)(zz[z >> 1] >> (16 * (z & 1))); }

RPV_INLINE int rpv_size(int v) {   // bit length of |v|
  const uint32_t a = (uint32_t)(v < 0 ? -v : v);
  return a ? 32 - __builtin_clz(a) : 0;
}
RPV_INLINE uint32_t rpv_value_bits(int v, int s) { return (uint32_t)(v < 0 ? v + (1 << s) - 1 : v) & ((1u << s) - 1u); }

// The symbols of one block into `sink`: sink.put(bits, n) appends the low n bits of `bits`, most significant first;
// n is at most 27.  get(z) is the block's coefficient at zigzag position z; pred the DC of the previous block of the
// component in this segment (0 for the first).
template <class Get, class Sink>
RPV_INLINE void rpv_walk(Get get, int pred, const uint32_t* dc, const uint32_t* ac, Sink& sink) {
  const int diff = get(0) - pred;
  int s = rpv_size(diff);
  uint32_t e = dc[s < 12 ? s : 11];
  sink.put(((e & 0xffffu) << s) | rpv_value_bits(diff, s), (int)(e >> 16) + s);
  const uint32_t zrl = ac[0xF0];
  int run = 0;
  for (int z = 1; z < 64; z++) {
    const int v = get(z);
    if (v == 0) { run++; continue; }
    for (; run > 15; run -= 16) sink.put(zrl & 0xffffu, (int)(zrl >> 16));
    s = rpv_size(v);
    s = s < 16 ? s : 15;
    e = ac[(run << 4) | s];
    sink.put(((e & 0xffffu) << s) | rpv_value_bits(v, s), (int)(e >> 16) + s);
    run = 0;
  }
  if (run > 0) sink.put(ac[0] & 0xffffu, (int)(ac[0] >> 16));
}

struct RpvCountSink {
  int bits = 0;
  RPV_INLINE void put(uint32_t, int n) { bits += n; }
};

// ---- the whole encoder on the host ----------------------------------------------------------------------------------
struct RpvHostBits {
  std::vector<unsigned char>& out;
  uint32_t acc = 0;
  int fill = 0;
  explicit RpvHostBits(std::vector<unsigned char>& o) : out(o) {}
  void byte(unsigned b) { out.push_back((unsigned char)b); if (b == 0xFF) out.push_back(0); }
  void put(uint32_t bits, int n) {
    for (int i = n - 1; i >= 0; i--) {
      acc = (acc << 1) | ((bits >> i) & 1u);
      if (++fill == 8) { byte(acc & 0xFF); acc = 0; fill = 0; }
    }
  }
  void pad() { while (fill) put(1, 1); }
};

// one frame's file into `file`
inline void rpv_encode_frame_host(const RpvTables& tab, const unsigned char* rgb, std::vector<unsigned char>& file) {
  const RpvGeom& G = tab.G;
  file.assign(tab.header.begin(), tab.header.end());
  for (int ty = 0; ty < G.nby; ty++) {
    RpvHostBits bw(file);
    int pred[3] = {0, 0, 0};
    for (int tx = 0; tx < G.nbx; tx++)
      for (int c = 0; c < 3; c++) {
        int X[64];
        uint32_t zz[32];
        rpv_load_block(rgb, G.H, G.W, ty, tx, c, X);
        rpv_transform_block(X, tab.quant.half[c ? 1 : 0], tab.quant.recip[c ? 1 : 0], zz);
        rpv_walk([&](int z) { return rpv_coef(zz, z); }, pred[c], tab.huff.dc[c ? 1 : 0], tab.huff.ac[c ? 1 : 0], bw);
        pred[c] = rpv_coef(zz, 0);
      }
    bw.pad();
    file.push_back(0xFF);
    file.push_back(ty == G.nby - 1 ? 0xD9 : (unsigned char)(0xD0 + (ty & 7)));
  }
}

// rp_video_encode with HOST pointers
inline void rpv_encode_host(const RpvTables& tab, const rp_video_encode_args* g) {
  std::vector<unsigned char> file;
  const size_t frame_bytes = (size_t)tab.G.H * tab.G.W * 3;
  for (int f = g->frame_first; f < g->frame_first + g->frame_count; f++) {
    rpv_encode_frame_host(tab, g->rgb + (size_t)f * frame_bytes, file);
    const size_t n = file.size() < (size_t)g->bytes_cap ? file.size() : (size_t)g->bytes_cap;
    memcpy(g->bytes + (size_t)f * g->bytes_cap, file.data(), n);
    g->length[f] = file.size() <= (size_t)g->bytes_cap ? (int)file.size() : -(int)file.size();
  }
}
