/* Host build of the DEVICE token math (pipelinerl_amd/csrc/prl_token_math.h) so that the exact
 * per-token formulas the HIP kernels execute can be checked against the oracle on a machine
 * without a GPU.  Test-only: nothing in the product links or calls this. */
#include "../../pipelinerl_amd/csrc/prl_token_math.h"

/* evaluates n masked tokens; out_* arrays have length n */
extern "C" void prl_host_token_eval(const prl_loss_config* cfg, long n, const float* nlp, const float* ent,
                         const float* old_lp, const float* ref_lp, const float* adv, const float* reward,
                         const float* group_tokens, const float* num_labels, const float* overflow,
                         float* contrib, float* g_nlp, float* g_ent, float* ratio_stat, float* kl,
                         float* clamp_no) {
  for (long i = 0; i < n; ++i) {
    PrlTokenIn x = {nlp[i], ent[i], old_lp[i], ref_lp[i], adv[i], reward[i], group_tokens[i], num_labels[i], overflow[i]};
    PrlTokenOut o;
    prl_token_eval(*cfg, x, o);
    contrib[i] = o.contrib;
    g_nlp[i] = o.g_nlp;
    g_ent[i] = o.g_ent;
    ratio_stat[i] = o.ratio_stat;
    kl[i] = o.kl;
    clamp_no[i] = o.clamp_no;
  }
}

/* every PrlTokenOut field of n arbitrary tokens (labelled or not: the kernel evaluates them all and selects afterwards);
 * out is [16][n] in the order of the struct, the three flags as 0.0 / 1.0 */
extern "C" void prl_host_token_eval_all(const prl_loss_config* cfg, long n, const float* nlp, const float* ent,
                         const float* old_lp, const float* ref_lp, const float* adv, const float* reward,
                         const float* group_tokens, const float* num_labels, const float* overflow, float* out) {
  for (long i = 0; i < n; ++i) {
    PrlTokenIn x = {nlp[i], ent[i], old_lp[i], ref_lp[i], adv[i], reward[i], group_tokens[i], num_labels[i], overflow[i]};
    PrlTokenOut o;
    prl_token_eval(*cfg, x, o);
    const float f[16] = {o.contrib, o.g_nlp, o.g_ent, o.w, o.A, o.ratio_stat, o.kl, o.kl_new_old, o.abs_lrno, o.exp_lrrn, o.exp_ref_old,
                         o.clamp_rn, o.clamp_no, (float)o.bad_nlp, (float)o.bad_lrrn, (float)o.bad_kl};
    for (int k = 0; k < 16; ++k) out[(long)k * n + i] = f[k];
  }
}
