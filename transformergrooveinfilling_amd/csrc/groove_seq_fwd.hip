// Translation unit of the sequence-resident forward kernels (gt_seq.h): every instantiation + its launcher.
#define GT_SEQ_TU_FWD
#include "gt_seq_inst.h"

void gt_seq_launch_pack(const SeqArgs& a, unsigned nblocks, hipStream_t s) { gt_launch(seq_pack_kernel, dim3(nblocks), dim3(256), s, a); }
int gt_seq_launch_fwd(const SeqArgs& a, const SeqKernelId& id, unsigned nblocks, hipStream_t s) {
  const dim3 grid(nblocks), block(GT_SEQ_NT);
  switch (gt_seq_kernel_key(id)) {
    GT_SEQ_QUAD_FWD(GT_SEQ_CASE_FWD)
    GT_SEQ_SPLIT(GT_SEQ_CASE_FWD)
    GT_SEQ_WHOLE(GT_SEQ_CASE_FWD)
  }
  return gt_seq_launch_fwd64(a, id, nblocks, s);      // (a translation unit of its own: groove_seq64.hip)
}
void gt_seq_launch_update_pack(const SeqArgs& a, int algo, float* params, float* grads, float* m, float* v, int64_t n, const gt_step_state* st,
                               int step_advanced, hipStream_t s) {
  const int64_t frags = (int64_t)a.L * a.kstride / 256;
  SeqUpd u{params, grads, m, v, n, st, algo, step_advanced, (int)((frags + 3) / 4),
           a.xchg >= 0 ? reinterpret_cast<const unsigned*>(a.ws + a.xchg) : nullptr};
  gt_launch(seq_update_pack_kernel, dim3((unsigned)(u.nblk_a + (n / 4 + 255) / 256 + 1)), dim3(256), s, a, u);
}
