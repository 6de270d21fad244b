// The K loop of the three MFMA GEMM kernels of csrc/pointwise_mfma.hip (forward / data gradient, its split-K form, weight
// gradient), included INSIDE each kernel body: acc = sum over the slabs [s_begin, s_end) of A-tile x B-tile.  Slab s lies in
// LDS buffer (s - s_begin) & 1; slab s + 1 travels global -> registers while s computes and is written to the other buffer
// after k-group kPwStashAt.  Text, not a function template: as a __forceinline__ template that takes the two steps as
// lambdas, the same loop compiled to a different instruction stream in all 54 instances (the slab loop peeled in the forward
// kernels, 164 -> 220 and 184 -> 240 VGPRs in the 128 x 128 weight gradient); this form compiles to what the three
// hand-kept copies did (profiles/pointwise_kloop_isa.md).
//
// Declared here: acc and the staging registers ra / ram (A and its mask), rb / rbm (B and its mask).  Names of the kernel
// used here: TM, TN, BK, BM, BN, As, Bs, t, wm, wn, lrow, lk, and
//   AMODE, BMODE           the operands' LDS images (kXC / kKC)
//   AMASK, BMASK           that operand carries a mask (applied by pw_stash)
//   BRELU                  B counts as relu(B)
//   EARLY                  write the next slab before the slab's last k-group (kPwStashAt)
//   MAY_BE_EMPTY           the slab range can be empty: then nothing is fetched and acc = 0
//   s_begin, s_end         the slab range
//   PW_K_SETUP             macro: declarations the steps below need, placed after the registers so that they can name them
//                          (the range too where the kernel has not declared it: where it is computed moves instructions)
//   PW_K_FETCH(s)          macro: slab s, global -> ra, ram, rb, rbm (two pw_fetch)
//   PW_K_SLAB_DONE(buf)    macro: after a slab's matrix instructions, its images still in As[buf] / Bs[buf]
  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
  PwRegs<PwImg<BM, BK, AMODE>::vecs> ra;
  PwRegs<PwImg<BN, BK, BMODE>::vecs> rb;
  PwRegs<AMASK ? PwImg<BM, BK, AMODE>::vecs : 1> ram;
  PwRegs<BMASK ? PwImg<BN, BK, BMODE>::vecs : 1> rbm;
  PW_K_SETUP
  if (!MAY_BE_EMPTY || s_begin < s_end) {
    PW_K_FETCH(s_begin);
    pw_stash<BM, BK, AMODE, AMASK>(As[0], ra, ram, t);
    pw_stash<BN, BK, BMODE, BMASK, BRELU>(Bs[0], rb, rbm, t);
  }
  __syncthreads();
  for (int s = s_begin; s < s_end; ++s) {
    const int buf = (s - s_begin) & 1;
    if (s + 1 < s_end) {                                // in flight while this slab computes
      PW_K_FETCH(s + 1);
    }
#pragma unroll
    for (int kg = 0; kg < BK / 8; ++kg) {
      float av[TM][4], bv[TN][4];
      pw_frag<TM, BM, BK, AMODE>(av, As[buf], wm * 32 * TM, kg, lrow, lk);
      pw_frag<TN, BN, BK, BMODE>(bv, Bs[buf], wn * 32 * TN, kg, lrow, lk);
      pw_mma<TM, TN>(acc, av, bv);
      if (kg == kPwStashAt(BK / 8, EARLY) && s + 1 < s_end) {
        // the next slab goes into the other buffer (nobody reads it in this step) while the matrix
        // core works through the instructions issued so far: the stores' latency is covered
        pw_stash<BM, BK, AMODE, AMASK>(As[buf ^ 1], ra, ram, t);
        pw_stash<BN, BK, BMODE, BMASK, BRELU>(Bs[buf ^ 1], rb, rbm, t);
      }
    }
    PW_K_SLAB_DONE(buf);
    if (s + 1 < s_end) __syncthreads();
  }
