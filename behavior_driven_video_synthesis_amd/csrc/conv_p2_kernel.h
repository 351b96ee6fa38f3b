// The two p2 convolution kernels (conv_p2.hip: layout, work decomposition, helpers), included ONCE PER TERM COUNT with P2_TERMS
// defined (no include guard).  Textual inclusion, not a term-count template parameter on a shared body: the two-term kernels
// keep their names (conv_p2_kernel<NW, CT, XBUF>, conv_p2a_kernel<CT> -- profiles, bench.py's roofline keys and
// vunet_p2_conv_variant spell them so) AND their exact device code (tools/device_asm_diff.sh); routing both term counts through
// one inlined body changed the register allocation of the existing instantiations.  The one-term kernels are overloads with
// one more template parameter (always 1): conv_p2_kernel<4, CT, 1, 1>, conv_p2_kernel<4, CT, 2, 1>, conv_p2a_kernel<CT, 1>.
//
// TERMS = 2: the arithmetic described above.  TERMS = 1 ("f16" mode of the perceptual loss, VUNET_TUNE_P2_TERMS): the hi
// plane of a planes tensor is by itself a complete scaled-fp16 image of it, so a one-term instantiation copies only the hi
// activation pieces and the hi weight slabs (read out of the SAME weight image with a stride of two slabs), reads only hi
// fragments and issues ONE product per tap into one accumulator set: half the bytes, a third of the matrix instructions,
// operands rounded to 11 bits.  Its epilogue is the two-term one: both output planes from the fp32 accumulators, the same
// bound, the same published maximum -- every consumer of the output sees the layout it sees today.
#if P2_TERMS == 2
template <int NW, int CT, int XBUF>
#else
template <int NW, int CT, int XBUF, int ONE>
#endif
__global__ __launch_bounds__(64 * NW, NW == 8 ? 1 : 2) void conv_p2_kernel(const P2Args a) {
  constexpr int TERMS = P2_TERMS;
  static_assert(NW == 4 || NW == 8, "waves");
  static_assert(CT == 32 || CT == 16, "tile width");
  static_assert(TERMS == 1 || TERMS == 2, "terms per operand");
  constexpr int MW = 16 * NW;                     // output channels of a workgroup
  constexpr int RT = 8, IH = RT + 2, CW = CT + 2, XPIX = IH * CW, XU = 4 * TERMS * XPIX;
  constexpr int NXI = (XU + 63) / 64, XS = NXI * 64;   // x tile of one chunk: wave-instructions / units incl. the overrun pad
  constexpr int NXW = (NXI + NW - 1) / NW;        // ... per wave
  constexpr int WU = MW * 4 * TERMS;              // units of a weight slab: [MW / 16 m-tiles][TERMS planes][64]
  constexpr int NWI = WU / 64 / NW;               // wave-instructions per wave and slab (= TERMS)
  constexpr int WSRC = TERMS == 2 ? 1024 : 2048;  // bytes between the image's 1 KiB pieces that are copied (one term: hi only)
  constexpr int PTR = CT / 16, NPT = 2 * PTR;     // 16-pixel tiles per tile row / per wave (two rows)
  static_assert(XBUF == 1 || NXW <= 8, "the next chunk's pieces ride on the first taps");
  extern __shared__ __attribute__((aligned(16))) uint4 smem[];
  uint4* const xL = smem;                // [XBUF][XS]
  uint4* const wL = smem + XBUF * XS;    // [2][WU]

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int mg = wave >> 2, rg = wave & 3;
  const int px = lane & 15, cg = lane >> 4;
  const int Hp = a.H + 2, Wp = a.W + 2, CB = a.C >> 3, MB = a.M >> 3;

  const unsigned bid = xcd_remap(blockIdx.x, gridDim.x);
  const int mblocks = a.M / MW;
  const int mb = bid % mblocks;
  int t = bid / mblocks;
  const int tiles_w = a.W / CT, tiles_h = a.H / RT;
  const int tx = t % tiles_w;
  t /= tiles_w;
  const int ty = t % tiles_h;
  const int n = t / tiles_h;
  const int row0 = ty * RT, col0 = tx * CT, m0 = mb * MW;

  // ---- chunk-invariant DMA geometry.  x: unit u of the tile = (plane, k-quarter, halo row, halo column); the tile's
  // origin in the PADDED map is (row0, col0) (its first halo row is padded row row0).  Byte offsets relative to the
  // (image, chunk) base; the wave-instructions past the end of the tile repeat its last piece (same bytes, same place).
  uint32_t xoff[NXW];
#pragma unroll
  for (int i = 0; i < NXW; ++i) {
    int j = wave + NW * i;
    if (j >= NXI) j = NXI - 1;
    int u = 64 * j + lane;
    if (u >= XU) u = XU - 1;             // (lands in the pad behind the tile)
    const int p = u / (4 * XPIX);
    int rem = u - p * 4 * XPIX;
    const int kq = rem / XPIX;
    rem -= kq * XPIX;
    const int r = rem / CW, c = rem - r * CW;
    xoff[i] = (uint32_t)((((size_t)p * a.N * CB + kq) * Hp + (row0 + r)) * Wp + col0 + c) * 16u;
  }
  const uint32_t xL_addr = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) void*)xL;
  const uint32_t wL_addr = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) void*)wL;
  const char* const xsrc0 = reinterpret_cast<const char*>(a.x) + (size_t)n * CB * Hp * Wp * 16;
  const size_t xchunk = (size_t)4 * Hp * Wp * 16;                  // bytes from one 32-channel chunk to the next
  const char* const wsrc0 = reinterpret_cast<const char*>(a.w) + (size_t)mb * (MW / 16) * 128 * 16;
  const size_t wslab = (size_t)(a.M / 16) * 128 * 16;             // bytes from one (chunk, tap) slab to the next
  const uint32_t lane16 = (uint32_t)lane * 16u;

  auto issue_x = [&](int ch, int i) {   // piece i of chunk ch's tile
    int j = wave + NW * i;
    if (j >= NXI) j = NXI - 1;
    if constexpr (TERMS == 1) j = __builtin_amdgcn_readfirstlane(j);   // (the clamp must not take the LDS address out of the SGPRs)
    const int xb = XBUF == 2 ? (ch & 1) : 0;
    p2_dma(xoff[i], p2_uniform_ptr(xsrc0 + (size_t)ch * xchunk), xL_addr + (uint32_t)(xb * XS + 64 * j) * 16u);
  };
  auto issue_w = [&](int g, int buf) {  // slab g = chunk * 9 + tap
    const char* src = wsrc0 + (size_t)g * wslab;
#pragma unroll
    for (int i = 0; i < NWI; ++i) {
      const int part = wave * NWI + i;
      p2_dma(lane16, p2_uniform_ptr(src + (size_t)part * WSRC), wL_addr + (uint32_t)(buf * WU + part * 64) * 16u);
    }
  };

  // ---- prologue: the first stage is requested at once, the scales are worked out behind it
  issue_w(0, 0);
#pragma unroll
  for (int i = 0; i < NXW; ++i) issue_x(0, i);

  float descale, descale2, sy;
  {
    const int ex = a.xmeta[0];
    const float amax_x = p2_meta_amax(a.xmeta, lane);
    const int ew = (int)a.wk[2];
    h2_pow2_pair(-(ex + ew), descale, descale2);
    const float bound = a.wk[0] * amax_x + a.wk[1];
    const int ey = h2_scale_exp(bound);
    sy = h2_pow2(ey);
    if (blockIdx.x == 0 && tid == 0) a.ymeta[0] = ey;
  }

  f32x4 acc[4][NPT], acx[4][NPT];   // leading term / the two cross terms (scaled by 2^11)
#pragma unroll
  for (int mt = 0; mt < 4; ++mt)
#pragma unroll
    for (int q = 0; q < NPT; ++q)
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[mt][q][r] = acx[mt][q][r] = 0.f;   // (one term: acx is never read)

  p2_dma_wait<0>();
  __syncthreads();

  const int nch = a.C >> 5;
  const uint4* const wA0 = wL + (mg * 4) * (64 * TERMS) + lane;             // + buf * WU + (mt * TERMS + plane) * 64
  const uint4* const xB0 = xL + cg * XPIX + px + (2 * rg) * CW;            // + xbuf * XS + plane * 4 * XPIX + (row + kh) * CW + col + kw

  auto chunk = [&](int ch, auto last_c) {
    constexpr bool LAST = decltype(last_c)::value;
    const uint4* const xB = xB0 + (XBUF == 2 ? (ch & 1) * XS : 0);
    const int wpar = (ch * 9) & 1;     // slab parity of this chunk's tap 0
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
      const int kh = tap / 3, kw = tap - 3 * kh;
      const int g = ch * 9 + tap;
      const int buf = wpar ^ (tap & 1);
      constexpr bool dummy = false;
      (void)dummy;
      const bool more_w = !(LAST && tap == 8);
      const bool xpiece = XBUF == 2 && !LAST && tap < NXW;
      if (more_w) issue_w(g + 1, buf ^ 1);      // (its buffer: slab g - 1, which every wave finished reading before the last barrier)
      if (xpiece) issue_x(ch + 1, tap);
      const uint4* const wA = wA0 + buf * WU;
      P2Unit av[TERMS][4], bv[TERMS][NPT];
#pragma unroll
      for (int p = 0; p < TERMS; ++p) {
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) av[p][mt].u = wA[(mt * TERMS + p) * 64];
#pragma unroll
        for (int q = 0; q < NPT; ++q) bv[p][q].u = xB[p * 4 * XPIX + (q / PTR + kh) * CW + (q % PTR) * 16 + kw];
      }
      // by product type: consecutive instructions never share an accumulator
      if constexpr (TERMS == 2) {
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
#pragma unroll
          for (int q = 0; q < NPT; ++q)
            acx[mt][q] = __builtin_amdgcn_mfma_f32_16x16x32_f16(av[TERMS - 1][mt].b, bv[0][q].b, acx[mt][q], 0, 0, 0);
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
#pragma unroll
          for (int q = 0; q < NPT; ++q)
            acx[mt][q] = __builtin_amdgcn_mfma_f32_16x16x32_f16(av[0][mt].b, bv[TERMS - 1][q].b, acx[mt][q], 0, 0, 0);
      }
#pragma unroll
      for (int mt = 0; mt < 4; ++mt)
#pragma unroll
        for (int q = 0; q < NPT; ++q)
          acc[mt][q] = __builtin_amdgcn_mfma_f32_16x16x32_f16(av[0][mt].b, bv[0][q].b, acc[mt][q], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
      if (more_w) {
        // the weight slab of the next tap was requested BEFORE this tap's x piece: waiting for all but the newest
        // transfer retires it (and the previous tap's piece) and leaves the piece a second tap to land
        if (xpiece) p2_dma_wait<1>();
        else p2_dma_wait<0>();
        __syncthreads();
        if (XBUF == 1 && tap == 8) {   // single x buffer: every wave is through with it -- refill, wait, publish
#pragma unroll
          for (int i = 0; i < NXW; ++i) issue_x(ch + 1, i);
          p2_dma_wait<0>();
          __syncthreads();
        }
      }
    }
  };
  for (int ch = 0; ch + 1 < nch; ++ch) chunk(ch, std::false_type{});
  chunk(nch - 1, std::true_type{});

  // ---- epilogue.  Accumulator tile (mt, q): lane (px, cg) holds channels m0 + 64 mg + 16 mt + 4 cg + {0..3} of pixel
  // (row0 + 2 rg + q / PTR, col0 + 16 (q % PTR) + px).  Pixel tiles are taken in pairs (q, q + 1): after the packed halves
  // have been exchanged between lane rows cg and cg ^ 1, the lanes of an even row hold the 8-channel unit of tile q, those of
  // the odd row the unit of tile q + 1 (channel block (cg >> 1) of the m-tile): one 16-byte store per plane.
  const bool relu = a.relu != 0;
  const size_t plane = (size_t)a.N * MB * Hp * Wp;    // units of one output plane
  float ymax = 0.f;
#pragma unroll
  for (int mt = 0; mt < 4; ++mt) {
    const int co = m0 + 64 * mg + 16 * mt + 4 * cg;
    float sh[4] = {0.f, 0.f, 0.f, 0.f};
    if (a.shift) {
      const float4 s4 = *reinterpret_cast<const float4*>(a.shift + co);
      sh[0] = s4.x; sh[1] = s4.y; sh[2] = s4.z; sh[3] = s4.w;
    }
#pragma unroll
    for (int qp = 0; qp < NPT; qp += 2) {
      uint32_t hh[2][2], ll[2][2];
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        float v[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float c;
          if constexpr (TERMS == 2) c = (acc[mt][qp + s][r] + acx[mt][qp + s][r] * (1.f / 2048.f)) * descale * descale2 + sh[r];
          else c = acc[mt][qp + s][r] * descale * descale2 + sh[r];
          c = (relu && !(c > 0.f)) ? 0.f : c;
          ymax = fmaxf(ymax, fabsf(c));
          v[r] = c * sy;
        }
        h2_split2(v[0], v[1], hh[s][0], ll[s][0]);
        h2_split2(v[2], v[3], hh[s][1], ll[s][1]);
      }
      p2_swap16(hh[0][0], hh[1][0]);
      p2_swap16(hh[0][1], hh[1][1]);
      p2_swap16(ll[0][0], ll[1][0]);
      p2_swap16(ll[0][1], ll[1][1]);
      uint4 uh = make_uint4(hh[0][0], hh[0][1], hh[1][0], hh[1][1]);
      uint4 ul = make_uint4(ll[0][0], ll[0][1], ll[1][0], ll[1][1]);
      const int q = qp + (cg & 1);
      const int orow = row0 + 2 * rg + q / PTR, ocol = col0 + (q % PTR) * 16 + px;
      const int cb = ((m0 + 64 * mg + 16 * mt) >> 3) + (cg >> 1);
      const size_t o = (((size_t)n * MB + cb) * Hp + (orow + 1)) * Wp + (ocol + 1);
      if (a.mask) {
        const uint4 mh = a.mask[o], ml = a.mask[plane + o];
        const uint32_t k0 = p2_nonzero_halves((mh.x | ml.x) & 0x7FFF7FFFu), k1 = p2_nonzero_halves((mh.y | ml.y) & 0x7FFF7FFFu);
        const uint32_t k2 = p2_nonzero_halves((mh.z | ml.z) & 0x7FFF7FFFu), k3 = p2_nonzero_halves((mh.w | ml.w) & 0x7FFF7FFFu);
        uh.x &= k0; uh.y &= k1; uh.z &= k2; uh.w &= k3;
        ul.x &= k0; ul.y &= k1; ul.z &= k2; ul.w &= k3;
      }
      a.y[o] = uh;
      a.y[plane + o] = ul;
    }
  }
  {
    const float m_ = wave_max(ymax);
    if (lane == 0)
      atomicMax(reinterpret_cast<unsigned*>(a.ymeta) + P2_AMAX0 + ((blockIdx.x * NW + wave) & (P2_NSLOT - 1)), __float_as_uint(m_));
  }
}

// ---- the eight-wave form with its two wave groups in ANTIPHASE.
// In conv_p2_kernel every wave of a workgroup reads its fragments right after the tap's barrier and multiplies afterwards:
// eight waves want 128 KB from the LDS at once (1024 cycles at 128 B / clock), the matrix pipes wait, then the LDS idles
// while 2 x 768 cycles of MFMAs run -- measured: the phases ADD (0.45 of the fp16 peak: 63 % pipe occupancy at the clock
// the chip holds).  Here waves 0-3 (one per SIMD) and waves 4-7 (their partners on the same SIMDs) run half a step apart:
//      group 0:  R(t) | M(t) | R(t+1) | M(t+1) | ...          R = the tap's 16 ds_read_b128 (+ issuing LDS-DMA),
//      group 1:   -   | R(t) | M(t)   | R(t+1) | ...          M = its 48 MFMAs;  "|" = s_barrier of all eight waves
// so that in every segment one wave of each SIMD multiplies while its partner reads.  One register set of fragments is
// enough (a wave's R segment starts after its M segment has ended).  Group 0 copies the weight slabs (slab t+1 at the start
// of R(t): its buffer was last read by group 1 one segment earlier, reads retired before that barrier), group 1 the next
// chunk's activation pieces; each group retires its own transfers at the end of its M segment, i.e. a full two segments
// after issuing them and one barrier before anybody reads them.  (Measured and not kept, r05: three slab buffers with the
// transfers requested two taps ahead and counted waits that leave the newest in flight -- conv4_x 173 us against 168 - 170:
// the transfers' latency is not what the loop waits for.)
//
// One term (TERMS = 1).  Nothing in the ordering argument above depends on how long a segment lasts: every hand-over is a
// retired wait followed by a barrier.  What changes is the balance -- R is 8 ds_read_b128 per wave (4 waves x 8 KiB = 256
// LDS cycles), M is 16 MFMAs (256 matrix-pipe cycles): the loop is read-bound where the two-term one is multiply-bound.
// LDS: 2 x (1408 | 768) x-units + 2 x 512 weight units = 60 | 40 KiB (CT = 32 | 16) against 118 | 78 KiB with two terms.
#if P2_TERMS == 2
template <int CT>
#else
template <int CT, int ONE>
#endif
__global__ __launch_bounds__(512, 1) void conv_p2a_kernel(const P2Args a) {
  constexpr int TERMS = P2_TERMS;
  static_assert(TERMS == 1 || TERMS == 2, "terms per operand");
  constexpr int NW = 8, MW = 128;
  constexpr int RT = 8, IH = RT + 2, CW = CT + 2, XPIX = IH * CW, XU = 4 * TERMS * XPIX;
  constexpr int NXI = (XU + 63) / 64, XS = NXI * 64;
  constexpr int NXG = (NXI + 3) / 4;               // x pieces per wave of group 1 and chunk
  constexpr int XPT = 2, NXT = (NXG + XPT - 1) / XPT;   // ... XPT per tap over the chunk's first NXT taps
  constexpr int WU = MW * 4 * TERMS;
  constexpr int WSRC = TERMS == 2 ? 1024 : 2048;
  constexpr int PTR = CT / 16, NPT = 2 * PTR;
  static_assert(NXT <= 8, "the next chunk's pieces must be visible before its first tap");
  extern __shared__ __attribute__((aligned(16))) uint4 smem[];
  uint4* const xL = smem;                // [2][XS]
  uint4* const wL = smem + 2 * XS;       // [2][WU]

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int mg = wave >> 2, rg = wave & 3;          // mg is also the wave's phase group
  const int px = lane & 15, cg = lane >> 4;
  const int Hp = a.H + 2, Wp = a.W + 2, CB = a.C >> 3, MB = a.M >> 3;

  const unsigned bid = xcd_remap(blockIdx.x, gridDim.x);
  const int mblocks = a.M / MW;
  const int mb = bid % mblocks;
  int t = bid / mblocks;
  const int tiles_w = a.W / CT, tiles_h = a.H / RT;
  const int tx = t % tiles_w;
  t /= tiles_w;
  const int ty = t % tiles_h;
  const int n = t / tiles_h;
  const int row0 = ty * RT, col0 = tx * CT, m0 = mb * MW;

  uint32_t xoff[NXG];                               // piece rg + 4 i of the tile (group 1; group 0 uses them in the prologue too)
#pragma unroll
  for (int i = 0; i < NXG; ++i) {
    int j = rg + 4 * i;
    if (j >= NXI) j = NXI - 1;
    int u = 64 * j + lane;
    if (u >= XU) u = XU - 1;
    const int p = u / (4 * XPIX);
    int rem = u - p * 4 * XPIX;
    const int kq = rem / XPIX;
    rem -= kq * XPIX;
    const int r = rem / CW, c = rem - r * CW;
    xoff[i] = (uint32_t)((((size_t)p * a.N * CB + kq) * Hp + (row0 + r)) * Wp + col0 + c) * 16u;
  }
  const uint32_t xL_addr = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) void*)xL;
  const uint32_t wL_addr = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) void*)wL;
  const char* const xsrc0 = reinterpret_cast<const char*>(a.x) + (size_t)n * CB * Hp * Wp * 16;
  const size_t xchunk = (size_t)4 * Hp * Wp * 16;
  const char* const wsrc0 = reinterpret_cast<const char*>(a.w) + (size_t)mb * (MW / 16) * 128 * 16;
  const size_t wslab = (size_t)(a.M / 16) * 128 * 16;
  const uint32_t lane16 = (uint32_t)lane * 16u;

  auto issue_x = [&](int ch, int i) {   // this wave's piece i of chunk ch (waves with the same rg copy the same piece)
    int j = rg + 4 * i;
    if (j >= NXI) j = NXI - 1;
    if constexpr (TERMS == 1) j = __builtin_amdgcn_readfirstlane(j);   // (the clamp must not take the LDS address out of the SGPRs)
    p2_dma(xoff[i], p2_uniform_ptr(xsrc0 + (size_t)ch * xchunk), xL_addr + (uint32_t)((ch & 1) * XS + 64 * j) * 16u);
  };
  auto issue_w = [&](int g, int buf) {  // this wave's quarter of slab g (four wave-instructions; one term: two)
    const char* src = wsrc0 + (size_t)g * wslab;
#pragma unroll
    for (int i = 0; i < 2 * TERMS; ++i) {
      const int part = rg * (2 * TERMS) + i;
      p2_dma(lane16, p2_uniform_ptr(src + (size_t)part * WSRC), wL_addr + (uint32_t)(buf * WU + part * 64) * 16u);
    }
  };

  // ---- prologue: group 0 requests slab 0, group 1 the first chunk's tile; the scales are worked out behind the transfers
  if (mg == 0) issue_w(0, 0);
  else {
#pragma unroll
    for (int i = 0; i < NXG; ++i) issue_x(0, i);
  }
  float descale, descale2, sy;
  {
    const int ex = a.xmeta[0];
    const float amax_x = p2_meta_amax(a.xmeta, lane);
    const int ew = (int)a.wk[2];
    h2_pow2_pair(-(ex + ew), descale, descale2);
    const float bound = a.wk[0] * amax_x + a.wk[1];
    const int ey = h2_scale_exp(bound);
    sy = h2_pow2(ey);
    if (blockIdx.x == 0 && tid == 0) a.ymeta[0] = ey;
  }
  f32x4 acc[4][NPT], acx[4][NPT];
#pragma unroll
  for (int mt = 0; mt < 4; ++mt)
#pragma unroll
    for (int q = 0; q < NPT; ++q)
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[mt][q][r] = acx[mt][q][r] = 0.f;   // (one term: acx is never read)
  p2_dma_wait<0>();
  __syncthreads();
  if (mg == 1) __builtin_amdgcn_s_barrier();       // group 1 runs one segment behind

  const int nch = a.C >> 5;
  const uint4* const wA0 = wL + (mg * 4) * (64 * TERMS) + lane;
  const uint4* const xB0 = xL + cg * XPIX + px + (2 * rg) * CW;

  auto chunk = [&](int ch, auto last_c) {
    constexpr bool LAST = decltype(last_c)::value;
    const uint4* const xB = xB0 + (ch & 1) * XS;
    const int wpar = (ch * 9) & 1;
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
      const int kh = tap / 3, kw = tap - 3 * kh;
      const int g = ch * 9 + tap;
      const int buf = wpar ^ (tap & 1);
      const bool more_w = !(LAST && tap == 8);
      // ---- R segment: request what the NEXT steps need, then read this tap's fragments
      if (mg == 0) {
        if (more_w) issue_w(g + 1, buf ^ 1);
      } else if (!LAST && tap < NXT) {
#pragma unroll
        for (int i = 0; i < XPT; ++i)
          if (tap * XPT + i < NXG) issue_x(ch + 1, tap * XPT + i);
      }
      const uint4* const wA = wA0 + buf * WU;
      P2Unit av[TERMS][4], bv[TERMS][NPT];
#pragma unroll
      for (int p = 0; p < TERMS; ++p) {
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) av[p][mt].u = wA[(mt * TERMS + p) * 64];
#pragma unroll
        for (int q = 0; q < NPT; ++q) bv[p][q].u = xB[p * 4 * XPIX + (q / PTR + kh) * CW + (q % PTR) * 16 + kw];
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // the reads are retired BEFORE the barrier: the partner group may refill
      __builtin_amdgcn_sched_barrier(0);
      __builtin_amdgcn_s_barrier();
      __builtin_amdgcn_sched_barrier(0);
      // ---- M segment
      __builtin_amdgcn_s_setprio(1);
      if constexpr (TERMS == 2) {
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
#pragma unroll
          for (int q = 0; q < NPT; ++q)
            acx[mt][q] = __builtin_amdgcn_mfma_f32_16x16x32_f16(av[TERMS - 1][mt].b, bv[0][q].b, acx[mt][q], 0, 0, 0);
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
#pragma unroll
          for (int q = 0; q < NPT; ++q)
            acx[mt][q] = __builtin_amdgcn_mfma_f32_16x16x32_f16(av[0][mt].b, bv[TERMS - 1][q].b, acx[mt][q], 0, 0, 0);
      }
#pragma unroll
      for (int mt = 0; mt < 4; ++mt)
#pragma unroll
        for (int q = 0; q < NPT; ++q)
          acc[mt][q] = __builtin_amdgcn_mfma_f32_16x16x32_f16(av[0][mt].b, bv[0][q].b, acc[mt][q], 0, 0, 0);
      __builtin_amdgcn_s_setprio(0);
      __builtin_amdgcn_sched_barrier(0);
      p2_dma_wait<0>();                                     // this wave's transfers of the R segment: landed
      __builtin_amdgcn_s_barrier();
      __builtin_amdgcn_sched_barrier(0);
    }
  };
  for (int ch = 0; ch + 1 < nch; ++ch) chunk(ch, std::false_type{});
  chunk(nch - 1, std::true_type{});
  if (mg == 0) __builtin_amdgcn_s_barrier();       // (both groups pass the same number of barriers)

  const bool relu = a.relu != 0;
  const size_t plane = (size_t)a.N * MB * Hp * Wp;
  float ymax = 0.f;
#pragma unroll
  for (int mt = 0; mt < 4; ++mt) {
    const int co = m0 + 64 * mg + 16 * mt + 4 * cg;
    float sh[4] = {0.f, 0.f, 0.f, 0.f};
    if (a.shift) {
      const float4 s4 = *reinterpret_cast<const float4*>(a.shift + co);
      sh[0] = s4.x; sh[1] = s4.y; sh[2] = s4.z; sh[3] = s4.w;
    }
#pragma unroll
    for (int qp = 0; qp < NPT; qp += 2) {
      uint32_t hh[2][2], ll[2][2];
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        float v[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float c;
          if constexpr (TERMS == 2) c = (acc[mt][qp + s][r] + acx[mt][qp + s][r] * (1.f / 2048.f)) * descale * descale2 + sh[r];
          else c = acc[mt][qp + s][r] * descale * descale2 + sh[r];
          c = (relu && !(c > 0.f)) ? 0.f : c;
          ymax = fmaxf(ymax, fabsf(c));
          v[r] = c * sy;
        }
        h2_split2(v[0], v[1], hh[s][0], ll[s][0]);
        h2_split2(v[2], v[3], hh[s][1], ll[s][1]);
      }
      p2_swap16(hh[0][0], hh[1][0]);
      p2_swap16(hh[0][1], hh[1][1]);
      p2_swap16(ll[0][0], ll[1][0]);
      p2_swap16(ll[0][1], ll[1][1]);
      uint4 uh = make_uint4(hh[0][0], hh[0][1], hh[1][0], hh[1][1]);
      uint4 ul = make_uint4(ll[0][0], ll[0][1], ll[1][0], ll[1][1]);
      const int q = qp + (cg & 1);
      const int orow = row0 + 2 * rg + q / PTR, ocol = col0 + (q % PTR) * 16 + px;
      const int cb = ((m0 + 64 * mg + 16 * mt) >> 3) + (cg >> 1);
      const size_t o = (((size_t)n * MB + cb) * Hp + (orow + 1)) * Wp + (ocol + 1);
      if (a.mask) {
        const uint4 mh = a.mask[o], ml = a.mask[plane + o];
        const uint32_t k0 = p2_nonzero_halves((mh.x | ml.x) & 0x7FFF7FFFu), k1 = p2_nonzero_halves((mh.y | ml.y) & 0x7FFF7FFFu);
        const uint32_t k2 = p2_nonzero_halves((mh.z | ml.z) & 0x7FFF7FFFu), k3 = p2_nonzero_halves((mh.w | ml.w) & 0x7FFF7FFFu);
        uh.x &= k0; uh.y &= k1; uh.z &= k2; uh.w &= k3;
        ul.x &= k0; ul.y &= k1; ul.z &= k2; ul.w &= k3;
      }
      a.y[o] = uh;
      a.y[plane + o] = ul;
    }
  }
  {
    const float m_ = wave_max(ymax);
    if (lane == 0)
      atomicMax(reinterpret_cast<unsigned*>(a.ymeta) + P2_AMAX0 + ((blockIdx.x * NW + wave) & (P2_NSLOT - 1)), __float_as_uint(m_));
  }
}
