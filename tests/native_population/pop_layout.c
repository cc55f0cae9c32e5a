/* TEST INFRASTRUCTURE ONLY: prints "name value" lines -- sizeof / offsetof of the population ABI's public
 * structs and QUADENV_ABI_VERSION -- as the C compiler lays include/quadenv.h out. */
#include <stddef.h>
#include <stdio.h>

#include "../../include/quadenv.h"

#define OFF(f) printf("offsetof_" #f " %zu\n", offsetof(QuadPopMember, f))

int main(void) {
  printf("abi_version %d\n", QUADENV_ABI_VERSION);
  printf("sizeof_QuadPopMember %zu\n", sizeof(QuadPopMember));
  printf("sizeof_QuadRollout %zu\n", sizeof(QuadRollout));
  printf("sizeof_QuadAdam %zu\n", sizeof(QuadAdam));
  OFF(env); OFF(params); OFF(grads); OFF(adam); OFF(packed); OFF(rollout); OFF(last_values); OFF(scratch_actions);
  OFF(advantages); OFF(returns); OFF(perm); OFF(adv_sums); OFF(mb_stats); OFF(workspace); OFF(workspace_bytes);
  OFF(gae_lambda); OFF(clip_range); OFF(ent_coef); OFF(vf_coef);
  printf("sizeof_QuadPopEval %zu\n", sizeof(QuadPopEval));
  printf("evaloffsetof_env %zu\n", offsetof(QuadPopEval, env));
  printf("evaloffsetof_run %zu\n", offsetof(QuadPopEval, run));
  printf("sizeof_QuadPolicyRun %zu\n", sizeof(QuadPolicyRun));
  return 0;
}
