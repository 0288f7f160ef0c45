// rp_video.hip -- librp_video.so: batched baseline-JPEG encoding of rendered frames (include/video/rp_video.h).
//
// Four launches per call, no global atomics:
//   rp_video_transform_kernel   one lane per 8 x 8 block (frame, tile row, tile, component): colour, padding, DCT and
//                               quantisation in registers; the coefficients leave in zigzag order as int16, one
//                               segment's blocks contiguous.
//   rp_video_entropy_kernel<0>  one wave per segment (MCU row), sizing: the wave walks the segment's blocks in chunks of
//                               RPV_CHUNK, one lane per block.  A lane stages its block in LDS (transposed, so the walk's
//                               run-time index costs no scratch), counts its bits, a DPP prefix sum gives its bit
//                               offset, and a second walk ors its codes into an LDS bit buffer (ds_or_b32; neighbouring
//                               lanes share words).  The chunk's whole bytes are then counted with their 0xFF stuffing
//                               (ballot + popcount); the bits of the last, partial byte are carried into the next chunk.
//                               Leaves the segment's stuffed size.
//   rp_video_layout_kernel      one wave per frame: exclusive scan of the segment sizes (+ 2 for each marker) gives every
//                               segment's place; writes the header and `length`.
//   rp_video_entropy_kernel<1>  the same walk again, now writing the stuffed bytes and the segment's marker in place.
// Every store into `bytes` is checked against bytes_cap.
#include "rp_abi_host.hpp"
#include "rp_video.hpp"

namespace {

#define RPV_TRANSFORM_THREADS 256
#define RPV_LDS_PITCH 65                                            /* words per coefficient pair: 64 lanes + 1, no bank conflicts */
#define RPV_BIT_WORDS ((RPV_CHUNK * RPV_BLOCK_BITS + 7 + 31) / 32 + 1)   /* a chunk's bits, the carried ones, one word of slack */

__global__ __launch_bounds__(RPV_TRANSFORM_THREADS, 2) void rp_video_transform_kernel(
    const RpvGeom G, const RpvQuant Q, const unsigned char* __restrict__ rgb, uint32_t* __restrict__ coef, int frame_first,
    long long n_blocks) {
  const long long gid = (long long)blockIdx.x * RPV_TRANSFORM_THREADS + threadIdx.x;
  if (gid >= n_blocks) return;
  // gid = ((frame * nby + ty) * nbx + tx) * 3 + comp, frame relative to the window
  const int comp = (int)(gid % 3);
  const long long tile = gid / 3;
  const int tx = (int)(tile % G.nbx);
  const long long row = tile / G.nbx;
  const int ty = (int)(row % G.nby);
  const long long frame = frame_first + row / G.nby;
  int X[64];
  rpv_load_block(rgb + (size_t)frame * G.H * G.W * 3, G.H, G.W, ty, tx, comp, X);
  uint32_t zz[32];
  const int t = comp ? 1 : 0;
  rpv_transform_block(X, Q.half[t], Q.recip[t], zz);
  uint4* dst = (uint4*)(coef + ((size_t)frame * G.nby * G.seg_blocks + (size_t)ty * G.seg_blocks + (size_t)tx * 3 + comp) * 32);
#pragma unroll
  for (int i = 0; i < 8; i++) dst[i] = make_uint4(zz[4 * i], zz[4 * i + 1], zz[4 * i + 2], zz[4 * i + 3]);
}

// inclusive prefix sum over the wave's 64 lanes: four row_shr steps scan each row of 16, row_bcast:15 adds row r - 1's
// total into rows 1 and 3, row_bcast:31 adds the total of rows 0 and 1 into rows 2 and 3
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ int dpp_add(int v) {
  return v + __builtin_amdgcn_update_dpp(0, v, CTRL, ROW_MASK, 0xf, ROW_MASK == 0xf);
}
__device__ __forceinline__ int wave_inclusive_scan(int v) {
  v = dpp_add<0x111, 0xf>(v);   // row_shr:1
  v = dpp_add<0x112, 0xf>(v);   // row_shr:2
  v = dpp_add<0x114, 0xf>(v);   // row_shr:4
  v = dpp_add<0x118, 0xf>(v);   // row_shr:8
  v = dpp_add<0x142, 0xa>(v);   // row_bcast:15 into rows 1 and 3 (the others keep `old` = 0)
  v = dpp_add<0x143, 0xc>(v);   // row_bcast:31 into rows 2 and 3
  return v;
}

struct LdsBitSink {   // a lane's codes into the chunk's bit buffer, most significant bit first
  uint32_t* buf;
  int pos;            // bit position of the next bit
  uint32_t cur;       // the bits gathered for word pos >> 5
  __device__ __forceinline__ void flush() { __hip_atomic_fetch_or(buf + (pos >> 5), cur, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
  __device__ __forceinline__ void put(uint32_t bits, int n) {
    if (n == 0) return;
    const int sh = pos & 31;
    const unsigned long long v = (unsigned long long)bits << (64 - n - sh);
    cur |= (uint32_t)(v >> 32);
    if (sh + n >= 32) { flush(); cur = (uint32_t)v; }
    pos += n;
  }
  __device__ __forceinline__ void finish() { if (cur) flush(); }
};

template <int WRITE>
__global__ __launch_bounds__(RPV_CHUNK) void rp_video_entropy_kernel(
    const RpvGeom G, const RpvHuff* __restrict__ huff, const uint32_t* __restrict__ coef, int* __restrict__ seg_len,
    const int* __restrict__ seg_off, unsigned char* __restrict__ bytes, int bytes_cap, int frame_first) {
  __shared__ uint32_t s_dc[2][12];
  __shared__ uint32_t s_ac[2][256];
  __shared__ uint32_t s_zz[32 * RPV_LDS_PITCH];
  __shared__ uint32_t s_bits[RPV_BIT_WORDS];
  const int lane = (int)threadIdx.x;
  const int seg = (int)(blockIdx.x % (unsigned)G.nby);
  const size_t frame = (size_t)frame_first + blockIdx.x / (unsigned)G.nby;
  const size_t fs = frame * G.nby + seg;
  const uint32_t* seg_coef = coef + fs * G.seg_blocks * 32;
  for (int i = lane; i < 24; i += RPV_CHUNK) (&s_dc[0][0])[i] = (&huff->dc[0][0])[i];
  for (int i = lane; i < 512; i += RPV_CHUNK) (&s_ac[0][0])[i] = (&huff->ac[0][0])[i];
  const unsigned long long below = (1ull << lane) - 1ull;
  unsigned char* out = bytes + frame * (size_t)bytes_cap;
  int out_pos = WRITE ? seg_off[fs] : 0;   // wave-uniform
  int carry_bits = 0;                      // 0..7 bits of the last, partial byte of the previous chunk ...
  uint32_t carry = 0;                      // ... in the low bits
  for (int b0 = 0; b0 < G.seg_blocks; b0 += RPV_CHUNK) {
    const int b = b0 + lane;
    const bool active = b < G.seg_blocks;
    const bool last = b0 + RPV_CHUNK >= G.seg_blocks;
    __syncthreads();   // the previous chunk's buffers have been read
    int pred = 0;
    if (active) {
      const uint4* src = (const uint4*)(seg_coef + (size_t)b * 32);
#pragma unroll
      for (int i = 0; i < 8; i++) {
        const uint4 w = src[i];
        s_zz[(4 * i) * RPV_LDS_PITCH + lane] = w.x; s_zz[(4 * i + 1) * RPV_LDS_PITCH + lane] = w.y;
        s_zz[(4 * i + 2) * RPV_LDS_PITCH + lane] = w.z; s_zz[(4 * i + 3) * RPV_LDS_PITCH + lane] = w.w;
      }
      if (b >= 3) pred = (int)(int16_t)(seg_coef[(size_t)(b - 3) * 32] & 0xffffu);   // a lookup, not a scan
    }
    const int t = (b % 3) ? 1 : 0;
    auto get = [&](int z) { return (int)(int16_t)(s_zz[(z >> 1) * RPV_LDS_PITCH + lane] >> (16 * (z & 1))); };
    // pass 1: bits per block, and where each lane's bits start
    RpvCountSink count;
    if (active) rpv_walk(get, pred, s_dc[t], s_ac[t], count);
    const int incl = wave_inclusive_scan(count.bits);
    const int total = carry_bits + __builtin_amdgcn_readlane(incl, 63);
    const int pad = last ? (8 - (total & 7)) & 7 : 0;
    const int n_words = (total + pad + 31) / 32 + 1;
    for (int i = lane; i < n_words; i += RPV_CHUNK) s_bits[i] = 0;
    __syncthreads();
    // pass 2: the codes
    LdsBitSink sink{s_bits, carry_bits + incl - count.bits, 0};
    if (lane == 0 && carry_bits) sink.cur = carry << (32 - carry_bits);
    if (active) rpv_walk(get, pred, s_dc[t], s_ac[t], sink);
    sink.finish();
    if (lane == 0 && pad) {
      LdsBitSink ones{s_bits, total, 0};
      ones.put((1u << pad) - 1u, pad);
      ones.finish();
    }
    __syncthreads();
    // the chunk's whole bytes, stuffed
    const int n_bytes = (total + pad) >> 3;
    carry_bits = (total + pad) & 7;
    carry = carry_bits ? ((s_bits[n_bytes >> 2] >> (24 - 8 * (n_bytes & 3))) & 0xffu) >> (8 - carry_bits) : 0u;
    for (int k0 = 0; k0 < n_bytes; k0 += RPV_CHUNK) {
      const int k = k0 + lane;
      const bool valid = k < n_bytes;
      const uint32_t byte = valid ? (s_bits[k >> 2] >> (24 - 8 * (k & 3))) & 0xffu : 0u;
      const bool ff = byte == 0xffu;
      const unsigned long long m = __ballot(ff);
      if (WRITE && valid) {
        const int o = out_pos + lane + __popcll(m & below);
        if (o < bytes_cap) out[o] = (unsigned char)byte;
        if (ff && o + 1 < bytes_cap) out[o + 1] = 0;
      }
      out_pos += (n_bytes - k0 < RPV_CHUNK ? n_bytes - k0 : RPV_CHUNK) + __popcll(m);
    }
  }
  if (WRITE) {
    if (lane == 0 && out_pos < bytes_cap) out[out_pos] = 0xff;
    if (lane == 1 && out_pos + 1 < bytes_cap) out[out_pos + 1] = seg == G.nby - 1 ? 0xd9 : (unsigned char)(0xd0 + (seg & 7));
  } else if (lane == 0) {
    seg_len[fs] = out_pos;
  }
}

__global__ __launch_bounds__(64) void rp_video_layout_kernel(
    const RpvGeom G, const unsigned char* __restrict__ header, const int* __restrict__ seg_len, int* __restrict__ seg_off,
    unsigned char* __restrict__ bytes, int bytes_cap, int* __restrict__ length, int frame_first) {
  const int lane = (int)threadIdx.x;
  const size_t frame = (size_t)frame_first + blockIdx.x;
  long long at = G.header_bytes;   // wave-uniform; a frame's bound fits an int (create), the sum is formed wider anyway
  for (int s0 = 0; s0 < G.nby; s0 += 64) {
    const int s = s0 + lane;
    const int n = s < G.nby ? seg_len[frame * G.nby + s] + 2 : 0;
    const int incl = wave_inclusive_scan(n);
    if (s < G.nby) seg_off[frame * G.nby + s] = (int)at + incl - n;
    at += __builtin_amdgcn_readlane(incl, 63);
  }
  unsigned char* out = bytes + frame * (size_t)bytes_cap;
  const int n_head = G.header_bytes < bytes_cap ? G.header_bytes : bytes_cap;
  for (int i = lane; i < n_head; i += 64) out[i] = header[i];
  if (lane == 0) length[frame] = at <= bytes_cap ? (int)at : -(int)at;
}

}  // namespace

struct rp_video {
  RpvTables tab;
  int max_frames = 0, device = 0;
  uint32_t* d_coef = nullptr;        // [max_frames][nby][seg_blocks][32]
  int* d_seg_len = nullptr;          // [max_frames][nby]
  int* d_seg_off = nullptr;          // [max_frames][nby]
  RpvHuff* d_huff = nullptr;
  unsigned char* d_header = nullptr;
};

extern "C" {

const char* rp_video_last_error(void) { return g_err.c_str(); }

int rp_video_create(int height, int width, int max_frames, int quality, int device, rp_video** out) {
  if (!out) return fail("rp_video_create: out is NULL");
  *out = nullptr;
  rp_video* v = new rp_video();
  const std::string err = v->tab.build(height, width, max_frames, quality);
  if (!err.empty()) { delete v; return fail("rp_video_create: " + err); }
  v->max_frames = max_frames; v->device = device;
  CreateGuard<rp_video> guard{v, rp_video_destroy};
  const RpvGeom& G = v->tab.G;
  const size_t n_seg = (size_t)max_frames * G.nby;
  HIP_OK_AS("rp_video_create", "hipSetDevice", hipSetDevice(device));
  HIP_OK_AS("rp_video_create", "hipMalloc", hipMalloc(&v->d_coef, n_seg * G.seg_blocks * 32 * sizeof(uint32_t)));
  HIP_OK_AS("rp_video_create", "hipMalloc", hipMalloc(&v->d_seg_len, n_seg * sizeof(int)));
  HIP_OK_AS("rp_video_create", "hipMalloc", hipMalloc(&v->d_seg_off, n_seg * sizeof(int)));
  if (upload("rp_video_create", &v->d_huff, &v->tab.huff, 1)) return -1;
  if (upload("rp_video_create", &v->d_header, v->tab.header.data(), v->tab.header.size())) return -1;
  *out = guard.release();
  return 0;
}

void rp_video_destroy(rp_video* v) {
  if (!v) return;
  (void)hipSetDevice(v->device);
  free_all({v->d_coef, v->d_seg_len, v->d_seg_off, v->d_huff, v->d_header});
  delete v;
}

int rp_video_encode(rp_video* v, const rp_video_encode_args* args) {
  RP_HANDLE_HEAD(v, "rp_video_encode: handle is NULL");
  RP_ARGS_CHECK(rpv_check_args(args, v->max_frames));
  HIP_OK(hipSetDevice(v->device));
  hipStream_t st = (hipStream_t)args->hip_stream;
  const RpvGeom& G = v->tab.G;
  // (create bounds max_frames x blocks per frame, so every grid below fits the x dimension)
  const long long n_blocks = (long long)args->frame_count * G.nby * G.seg_blocks;
  const unsigned n_seg = (unsigned)(args->frame_count * G.nby);
  hipLaunchKernelGGL(rp_video_transform_kernel, dim3((unsigned)((n_blocks + RPV_TRANSFORM_THREADS - 1) / RPV_TRANSFORM_THREADS)),
                     dim3(RPV_TRANSFORM_THREADS), 0, st, G, v->tab.quant, args->rgb, v->d_coef, args->frame_first, n_blocks);
  HIP_OK(hipGetLastError());
  hipLaunchKernelGGL(rp_video_entropy_kernel<0>, dim3(n_seg), dim3(RPV_CHUNK), 0, st, G, (const RpvHuff*)v->d_huff,
                     (const uint32_t*)v->d_coef, v->d_seg_len, (const int*)v->d_seg_off, args->bytes, args->bytes_cap,
                     args->frame_first);
  HIP_OK(hipGetLastError());
  hipLaunchKernelGGL(rp_video_layout_kernel, dim3((unsigned)args->frame_count), dim3(64), 0, st, G,
                     (const unsigned char*)v->d_header, (const int*)v->d_seg_len, v->d_seg_off, args->bytes, args->bytes_cap,
                     args->length, args->frame_first);
  HIP_OK(hipGetLastError());
  hipLaunchKernelGGL(rp_video_entropy_kernel<1>, dim3(n_seg), dim3(RPV_CHUNK), 0, st, G, (const RpvHuff*)v->d_huff,
                     (const uint32_t*)v->d_coef, v->d_seg_len, (const int*)v->d_seg_off, args->bytes, args->bytes_cap,
                     args->frame_first);
  HIP_OK(hipGetLastError());
  return 0;
}

int rp_video_max_bytes(const rp_video* v) { return v ? (int)v->tab.max_bytes : -1; }

int rp_video_header(const rp_video* v, unsigned char* dst, int* n) {
  if (!v || !n) return fail("rp_video_header: handle or n is NULL");
  const int have = (int)v->tab.header.size();
  if (dst) memcpy(dst, v->tab.header.data(), (size_t)(*n < have ? (*n < 0 ? 0 : *n) : have));
  *n = have;
  return 0;
}

int rp_video_dim(const rp_video* v, const char* name) {
  if (!v || !name) return -1;
  if (!strcmp(name, "height")) return v->tab.G.H;
  if (!strcmp(name, "width")) return v->tab.G.W;
  if (!strcmp(name, "max_frames")) return v->max_frames;
  if (!strcmp(name, "quality")) return v->tab.quality;
  if (!strcmp(name, "segments")) return v->tab.G.nby;
  if (!strcmp(name, "segment_blocks")) return v->tab.G.seg_blocks;
  if (!strcmp(name, "chunk_blocks")) return RPV_CHUNK;
  return -1;
}

}  // extern "C"
