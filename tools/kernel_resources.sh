#!/bin/bash
# Per-kernel VGPRs, AGPRs, scratch bytes per lane, waves per SIMD and LDS bytes per block of the product TUs
# (compiler remarks), one line per kernel: unit kernel VGPRs AGPRs scratch waves/SIMD LDS
#   tools/kernel_resources.sh <dir holding csrc/>   (diff two trees to see what a change costs)
# The policy and critic kernels are among them: the ObsPol / ObsPolV instantiations of the two rollout
# units and their sampled siblings ObsPolS / ObsPolVS, policy.hip's policy_flock_kernel,
# policy_flock_sampled_kernel, policy_noise_kernel, value_flock_kernel and gae_kernel, and policy_grad.hip's
# mlp_grad_kernel, mlp_ppo_grad_kernel and mlp_ppo_grad_rows_kernel (one wave per block: waves per CU =
# 4 x waves/SIMD) and mlp_grad_reduce_kernel, and ppo_loss.hip's policy_logp_kernel, ppo_loss_kernel,
# ppo_stats_kernel, adv_sum_kernel and adv_finish_kernel, ppo_adam.hip's ppo_adam_kernel (one workgroup), and
# tdm_policy_grad.hip's tdm_policy_grad_kernel (one wave per block) and tdm_grad_reduce_kernel.
cd $1
for f in csrc/flock_step_w64.hip csrc/flock_rollout_w64.hip csrc/flock_rollout_ar_w64.hip csrc/flock_step_wg.hip csrc/tdm_step_wg.hip csrc/policy.hip csrc/policy_grad.hip csrc/ppo_loss.hip csrc/ppo_adam.hip csrc/tdm_policy_grad.hip; do
  extra=""; case $f in csrc/flock_rollout_w64.hip|csrc/flock_rollout_ar_w64.hip) extra="-mllvm -disable-machine-licm";; esac
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -fno-slp-vectorize $extra -Rpass-analysis=kernel-resource-usage -c -o /dev/null $f 2>&1 | grep -E "Function Name|VGPRs:|AGPRs:|ScratchSize|Occupancy|LDS Size" | paste - - - - - - | sed -E 's/.*Function Name: ([^ ]*).*VGPRs: ([0-9]+).*AGPRs: ([0-9]+).*lane\]: ([0-9]+).*SIMD\]: ([0-9]+).*block\]: ([0-9]+).*/\1 \2 \3 \4 \5 \6/' | sed "s#^#$(basename $f) #"
done
