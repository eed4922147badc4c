// update_launch.inc -- the (VEC, LPR, OPT) dispatch of the update kernels, included by update.hip (DCTR_UPD_GEN false) and
// update_gen.hip (true) inside a function that has `a`, `vec`, `lpr`, `opt`, `grid`, `block`, `s` in scope.
// presorted: one launch -- the lean path for every partition the pre-pass could sort, the general path inside the same
// kernel for an overflowing one, the dense half of Linear in the first workgroups (`grid` already counts them).  Otherwise
// the general kernel (every workgroup scans or takes its bucket, and sorts).
#define DCTR_UPD_PAIR(VEC_, LPR_, OPT_)                                                      \
  do {                                                                                       \
    if (a.presorted) {                                                                       \
      k_embed_apply_sorted<VEC_, LPR_, OPT_, DCTR_UPD_GEN><<<grid, block, 0, s>>>(a);        \
    } else {                                                                                 \
      k_embed_update<VEC_, LPR_, OPT_, DCTR_UPD_GEN><<<grid, block, 0, s>>>(a);              \
    }                                                                                        \
  } while (0)
// (DCTR_UPD_LAZY: simple units and pre-sorted entries only -- update.hip; update_gen.hip never sees it)
#if DCTR_UPD_GEN
#define DCTR_UPD_LAZY_LAUNCH(VEC_, LPR_) return DCTR_ENOSUP
#else
#define DCTR_UPD_LAZY_LAUNCH(VEC_, LPR_) k_embed_apply_sorted<VEC_, LPR_, 3, false><<<grid, block, 0, s>>>(a)
#endif
#define DCTR_UPD_LAUNCH(VEC_, LPR_)                                    \
  do {                                                                 \
    if (opt == DCTR_UPD_ADAGRAD) DCTR_UPD_PAIR(VEC_, LPR_, 1);         \
    else if (opt == DCTR_UPD_SGD) DCTR_UPD_PAIR(VEC_, LPR_, 0);        \
    else if (opt == DCTR_UPD_LAZY) DCTR_UPD_LAZY_LAUNCH(VEC_, LPR_);   \
    else DCTR_UPD_PAIR(VEC_, LPR_, 2);                                 \
  } while (0)

#define DCTR_UPD_LPR(VEC_)                      \
  switch (lpr) {                                \
    case 1: DCTR_UPD_LAUNCH(VEC_, 1); break;    \
    case 2: DCTR_UPD_LAUNCH(VEC_, 2); break;    \
    case 4: DCTR_UPD_LAUNCH(VEC_, 4); break;    \
    case 8: DCTR_UPD_LAUNCH(VEC_, 8); break;    \
    case 16: DCTR_UPD_LAUNCH(VEC_, 16); break;  \
    case 32: DCTR_UPD_LAUNCH(VEC_, 32); break;  \
    default: DCTR_UPD_LAUNCH(VEC_, 64); break;  \
  }
#define DCTR_UPD_LPR8()                       \
  switch (lpr) {                              \
    case 1: DCTR_UPD_LAUNCH(8, 1); break;     \
    case 2: DCTR_UPD_LAUNCH(8, 2); break;     \
    case 4: DCTR_UPD_LAUNCH(8, 4); break;     \
    default: DCTR_UPD_LAUNCH(8, 8); break;    \
  }
  if (vec == 8) { DCTR_UPD_LPR8() } else if (vec == 4) { DCTR_UPD_LPR(4) } else if (vec == 2) { DCTR_UPD_LPR(2) } else { DCTR_UPD_LPR(1) }
#undef DCTR_UPD_PAIR
#undef DCTR_UPD_LAUNCH
#undef DCTR_UPD_LAZY_LAUNCH
#undef DCTR_UPD_LPR
#undef DCTR_UPD_LPR8
