// sph_video.hpp -- video encoding (one RGB frame on the device -> the entropy-coded scan of a baseline JPEG): kernels and launchers;
// included by sph_kernels.hip inside the per-build namespace.  The stream and every fixed-point format are defined in DESIGN.md 18,
// the entry points in include/sph_hip.h (sph_video_create), the restatement in tests/jpeg_model.py.  Integer arithmetic only: the strict
// and the fast build write the same bytes.
//
// One workgroup (4 waves) per restart interval of VIDEO_RI MCUs, one wave per 8x8 block, lane = sample, then = coefficient:
//   transform  lane (r, c) converts its pixel(s) to a level-shifted sample with 16 fraction bits; the row pass and the column pass are
//              8 multiply-adds each on values fetched by shuffles (64-bit sums, matrix with 20 fraction bits, each pass rounded back to
//              16); the lane quantises its coefficient and files it at its zigzag position in LDS
//   symbols    lane k holds zigzag coefficient k (lane 0: the DC difference to the component's previous block of the interval, read
//              from LDS).  The ballot of the non-zero lanes gives each its zero run (and the lane that appends EOB), so every lane forms
//              its own bits -- ZRLs, Huffman code, magnitude bits, at most 63 -- with no loop over the block
//   layout     the lanes' bit counts scanned in the wave, the blocks' totals scanned by wave 0: every lane knows its bit offset in the
//              interval and ORs its bits into the interval's LDS image (OR commutes: the image is independent of the order)
//   bytes      the image padded with ones to a byte; a workgroup scan over the 0xFF flags places every byte behind the stuffed zeros
//              before it; the interval's marker RSTn follows (not after the last interval)
// The kernel runs twice per frame: COUNT leaves the interval's byte count (l_video_scan: exclusive scan, the total at the end, which
// the host reads to size the output exactly), WRITE computes the same bytes again and stores them at the scanned offset.  Nothing is
// sized by a guess, nothing is truncated; the only worst case used is the LDS image's (VIDEO_BLOCK_BITS, from the tables).
#pragma once

#define VIDEO_MAXBLK (VIDEO_RI * 6)   // blocks of an interval (4:2:0: 6 per MCU, 4:4:4: 3): <= 64, one wave scans their totals
// the most bits a block can take: DC code + magnitude <= 11 + 11, and per AC position at most the longest code + magnitude, 16 + 10
// (a ZRL's 11 bits stand for 16 positions, an EOB's 4 for at least one)
#define VIDEO_BLOCK_BITS (22 + 63 * 26)
#define VIDEO_WORDS ((VIDEO_MAXBLK * VIDEO_BLOCK_BITS + 31) / 32 + 3)   // + the two words a lane's bits can spill into, + padding
static_assert(VIDEO_MAXBLK <= 64, "one wave scans the block totals of an interval");

// round(2^20 a(u) cos((2x + 1) u pi / 16)), a(0) = sqrt(1/8), a(u) = 1/2: row u, column x (no entry is nearer than
// 0.014 to a rounding tie)
static __device__ const int VIDEO_C[64] = {
    370728, 370728, 370728, 370728, 370728, 370728, 370728, 370728,
    514214, 435930, 291279, 102284, -102284, -291279, -435930, -514214,
    484379, 200636, -200636, -484379, -484379, -200636, 200636, 484379,
    435930, -102284, -514214, -291279, 291279, 514214, 102284, -435930,
    370728, -370728, -370728, 370728, 370728, -370728, -370728, 370728,
    291279, -514214, 102284, 435930, -435930, -102284, 514214, -291279,
    200636, -484379, 484379, -200636, -200636, 484379, -484379, 200636,
    102284, -291279, 435930, -514214, 514214, -435930, 291279, -102284};
// natural index (8 u + v) -> zigzag position (T.81 figure A.6)
static __device__ const unsigned char VIDEO_ZZ[64] = {
    0, 1, 5, 6, 14, 15, 27, 28,
    2, 4, 7, 13, 16, 26, 29, 42,
    3, 8, 12, 17, 25, 30, 41, 43,
    9, 11, 18, 24, 31, 40, 44, 53,
    10, 19, 23, 32, 39, 45, 52, 54,
    20, 22, 33, 38, 46, 51, 55, 60,
    21, 34, 37, 47, 50, 56, 59, 61,
    35, 36, 48, 49, 57, 58, 62, 63};

// one pixel, clamped to the picture (the padding repeats the last column and row), as component comp with 16 fraction bits
__device__ __forceinline__ int video_ycc(const VideoDev &d, int x, int y, int comp) {
    x = min(x, d.W - 1); y = min(y, d.H - 1);
    const unsigned char *p = d.rgb + 3 * ((size_t)y * d.W + x);
    const int r = p[0], g = p[1], b = p[2];
    if (comp == 0) return 19595 * r + 38470 * g + 7471 * b - (128 << 16);
    if (comp == 1) return -11058 * r - 21710 * g + 32768 * b;
    return 32768 * r - 27439 * g - 5329 * b;
}

// sample (r, c) of block k of MCU (mx, my)
__device__ __forceinline__ int video_sample(const VideoDev &d, int mx, int my, int k, int comp, int r, int c) {
    if (!d.c420) return video_ycc(d, mx * 8 + c, my * 8 + r, comp);
    if (comp == 0) return video_ycc(d, mx * 16 + (k & 1) * 8 + c, my * 16 + (k >> 1) * 8 + r, 0);
    const int x = mx * 16 + 2 * c, y = my * 16 + 2 * r;
    return (video_ycc(d, x, y, comp) + video_ycc(d, x + 1, y, comp) + video_ycc(d, x, y + 1, comp) + video_ycc(d, x + 1, y + 1, comp) + 2) >> 2;
}

__device__ __forceinline__ int video_wave_sum(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// The bits of zigzag position `lane` of one block, right-aligned in code, and their number: v = the quantised coefficient (lane 0: the
// DC difference), nz = the ballot of the non-zero positions with bit 0 set (the DC is always coded), tc = 0 luminance / 1 chrominance
// tables.  A table entry is code | length << 16.
__device__ __forceinline__ void video_symbol(const VideoTables *T, int tc, int lane, int v, unsigned long long nz,
                                             unsigned long long &code, int &len) {
    code = 0; len = 0;
    const int a = v < 0 ? -v : v;
    const int size = 32 - __clz(a);
    const unsigned mag = (unsigned)(v < 0 ? v - 1 : v) & ((1u << size) - 1u);
    if (lane == 0) {
        const unsigned h = T->dc[tc][size];
        code = ((unsigned long long)(h & 0xffffu) << size) | mag;
        len = (int)(h >> 16) + size;
    } else if (v != 0) {
        const int prev = 63 - __clzll((long long)(nz & ((1ull << lane) - 1ull)));   // the non-zero position before this one (0: the DC)
        const int run = lane - prev - 1;
        const unsigned z = T->ac[tc][0xF0];
        for (int k = run >> 4; k > 0; --k) { code = (code << (z >> 16)) | (z & 0xffffu); len += (int)(z >> 16); }
        const unsigned h = T->ac[tc][((run & 15) << 4) | size];
        code = (code << ((h >> 16) + size)) | ((unsigned long long)(h & 0xffffu) << size) | mag;
        len += (int)(h >> 16) + size;
    }
    const int last = 63 - __clzll((long long)nz);
    if (lane == last && last < 63) {   // zeros to the end of the block: EOB behind the last coded position
        const unsigned e = T->ac[tc][0];
        code = (code << (e >> 16)) | (e & 0xffffu);
        len += (int)(e >> 16);
    }
}

// block j of an interval: its place in the MCU, its component, and the block before it of that component (-1: the interval's first)
struct VideoBlk { int k, comp, prev; };
__device__ __forceinline__ VideoBlk video_blk(const VideoDev &d, int j) {
    const int bpm = d.c420 ? 6 : 3, m = j / bpm;
    VideoBlk b;
    b.k = j - m * bpm;
    b.comp = d.c420 ? (b.k < 4 ? 0 : b.k - 3) : b.k;
    if (d.c420 && b.comp == 0 && b.k > 0) b.prev = j - 1;
    else b.prev = m > 0 ? (m - 1) * bpm + (d.c420 && b.comp == 0 ? 3 : b.k) : -1;
    return b;
}

// lane's coefficient of block j, the ballot, and its bits
__device__ __forceinline__ void video_lane_bits(const VideoDev &d, const short (*coef)[64], int j, int lane, unsigned long long &code, int &len) {
    const VideoBlk b = video_blk(d, j);
    int v = coef[j][lane];
    const unsigned long long nz = __ballot(v != 0) | 1ull;
    if (lane == 0 && b.prev >= 0) v -= coef[b.prev][0];
    video_symbol(d.tab, b.comp ? 1 : 0, lane, v, nz, code, len);
}

template <bool WRITE>
__global__ void __launch_bounds__(256) k_video_interval(VideoDev d) {
    __shared__ short s_coef[VIDEO_MAXBLK][64];
    __shared__ unsigned s_bits[VIDEO_WORDS];
    __shared__ int s_boff[VIDEO_MAXBLK + 1];
    __shared__ int s_w[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int bpm = d.c420 ? 6 : 3;
    const int m0 = blockIdx.x * VIDEO_RI;
    const int nblk = min(VIDEO_RI, d.nmcu - m0) * bpm;

    // transform and quantisation
    for (int j = wave; j < nblk; j += 4) {
        const VideoBlk b = video_blk(d, j);
        const int m = m0 + j / bpm;
        const int s = video_sample(d, m % d.mw, m / d.mw, b.k, b.comp, lane >> 3, lane & 7);
        long long acc = 0;
#pragma unroll
        for (int x = 0; x < 8; ++x) acc += (long long)__shfl(s, (lane & 56) | x, 64) * VIDEO_C[(lane & 7) * 8 + x];
        const int t = (int)((acc + (1 << 19)) >> 20);   // row pass: lane (r, v), 16 fraction bits
        acc = 0;
#pragma unroll
        for (int y = 0; y < 8; ++y) acc += (long long)__shfl(t, y * 8 + (lane & 7), 64) * VIDEO_C[(lane >> 3) * 8 + y];
        const int f = (int)((acc + (1 << 19)) >> 20);   // coefficient (u, v) = lane, 16 fraction bits
        const unsigned D = (unsigned)d.tab->q[b.comp ? 1 : 0][lane] << 16;
        const unsigned a = (unsigned)(f < 0 ? -f : f);
        const int q = (int)((a + (D >> 1)) / D);        // half away from zero, straight from the fixed-point coefficient
        s_coef[j][VIDEO_ZZ[lane]] = (short)(f < 0 ? -q : q);
    }
    __syncthreads();

    // bits per block, their scan
    for (int j = wave; j < nblk; j += 4) {
        unsigned long long code; int len;
        video_lane_bits(d, s_coef, j, lane, code, len);
        len = video_wave_sum(len);
        if (lane == 0) s_boff[j] = len;
    }
    __syncthreads();
    if (wave == 0) {
        const int v = lane < nblk ? s_boff[lane] : 0;
        const int inc = wave_incl_scan(v);
        if (lane < nblk) s_boff[lane] = inc - v;
        if (lane == 63) s_boff[VIDEO_MAXBLK] = inc;
    }
    __syncthreads();
    const int tb = s_boff[VIDEO_MAXBLK];   // bits of the interval
    for (int w = tid; w < ((tb + 31) >> 5) + 3; w += 256) s_bits[w] = 0u;
    __syncthreads();

    // the interval's image, MSB first: bit o of the interval is bit 31 - (o & 31) of word o >> 5
    for (int j = wave; j < nblk; j += 4) {
        unsigned long long code; int len;
        video_lane_bits(d, s_coef, j, lane, code, len);
        const int o = s_boff[j] + wave_incl_scan(len) - len;
        if (len > 0) {
            const unsigned long long v = code << (64 - len);   // left-aligned
            const int w = o >> 5, sh = o & 31;
            const unsigned long long hi = v >> sh;
            const unsigned w0 = (unsigned)(hi >> 32), w1 = (unsigned)hi, w2 = sh ? (unsigned)((v << (64 - sh)) >> 32) : 0u;
            if (w0) atomicOr(&s_bits[w], w0);
            if (w1) atomicOr(&s_bits[w + 1], w1);
            if (w2) atomicOr(&s_bits[w + 2], w2);
        }
    }
    const int pad = -tb & 7;   // ones up to the byte boundary (inside one byte, so inside one word)
    if (tid == 0 && pad) atomicOr(&s_bits[tb >> 5], ((1u << pad) - 1u) << (32 - (tb & 31) - pad));
    __syncthreads();

    // bytes, each behind the zeros stuffed before it
    const int n = (tb + 7) >> 3;
    const size_t base = WRITE ? (size_t)d.len[blockIdx.x] : 0;
    int stuffed = 0;
    for (int c0 = 0; c0 < n; c0 += 256) {
        const int i = c0 + tid;
        unsigned b = 0u;
        if (i < n) b = (s_bits[i >> 2] >> (24 - 8 * (i & 3))) & 0xffu;
        const bool ff = i < n && b == 0xffu;
        int tot;
        const int before = block_excl_scan_256(ff ? 1 : 0, s_w, tot);
        if (WRITE && i < n) {
            const size_t o = base + (size_t)(i + stuffed + before);
            d.out[o] = (unsigned char)b;
            if (ff) d.out[o + 1] = 0;
        }
        stuffed += tot;
    }
    if (tid == 0) {
        const bool last = (int)blockIdx.x == d.nint - 1;
        if (WRITE) {
            if (!last) { d.out[base + n + stuffed] = 0xff; d.out[base + n + stuffed + 1] = (unsigned char)(0xd0 + (blockIdx.x & 7)); }
        } else {
            d.len[blockIdx.x] = n + stuffed + (last ? 0 : 2);
            if (stuffed) atomicAdd(&d.cnt[0], (unsigned long long)stuffed);
        }
    }
}

// exclusive scan of a[0, n) in place, a[n] = the total: one workgroup walks the array.  n = the restart intervals of a frame: 512 at
// 1024^2 4:2:0 (two trips of the loop), at most 131072 + edge MCUs at the 2^26 pixels sph_video_create accepts (about 520 trips, next
// to a count pass over 2^26 pixels); the tiled scan of sph_device.hpp is built around the cell grid's banks and statistics slots.
// The offsets are int: a block takes at most VIDEO_BLOCK_BITS bits, every byte can be stuffed, every interval adds a marker
__global__ void __launch_bounds__(256) k_video_scan(int *a, int n) {
    __shared__ int s_w[4];
    int run = 0;
    for (int c0 = 0; c0 < n; c0 += 256) {
        const int i = c0 + (int)threadIdx.x;
        const int v = i < n ? a[i] : 0;
        int tot;
        const int ex = block_excl_scan_256(v, s_w, tot);
        if (i < n) a[i] = run + ex;
        run += tot;
    }
    if (threadIdx.x == 0) a[n] = run;
}

// most blocks of a frame: 4:4:4, 2^26 pixels in 8 x 8 MCUs plus one MCU row and column of padding at 16384 pixels a side
static_assert((3LL * ((1LL << 26) / 64 + 2 * (16384 / 8) + 1)) * (2 * ((VIDEO_BLOCK_BITS + 7) / 8)) + 2 * (((1LL << 26) / 64) / VIDEO_RI + 2) < 2147483647LL,
              "the scan bytes of the largest frame fit an int");
static void l_video_count(VideoDev &d) { hipLaunchKernelGGL(k_video_interval<false>, dim3(d.nint), dim3(256), 0, d.stream, d); }
static void l_video_scan(VideoDev &d) { hipLaunchKernelGGL(k_video_scan, dim3(1), dim3(256), 0, d.stream, d.len, d.nint); }
static void l_video_write(VideoDev &d) { hipLaunchKernelGGL(k_video_interval<true>, dim3(d.nint), dim3(256), 0, d.stream, d); }

static void register_video_launchers(Launch &L) {
    L.video_count = l_video_count;
    L.video_scan = l_video_scan;
    L.video_write = l_video_write;
}
