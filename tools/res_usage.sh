#!/bin/bash
# Register / scratch usage of the v2 step kernel instantiations (compile-only, host side).
# usage: tools/res_usage.sh [source]   (default rl-cattle-herding_amd/csrc/ch_step.hip: k_step2, k_step2_actor)
# For k_step2_multi pass csrc/ch_step_multi.hip with its per-source flags (cattleherd/_build.py SOURCE_FLAGS):
#   EXTRA="-mllvm -disable-machine-licm" tools/res_usage.sh rl-cattle-herding_amd/csrc/ch_step_multi.hip
# The step itself (step2_body) is in csrc/ch_step_body.h, which both sources include (its sync primitives and flock math:
# ch_step_sync.h, ch_step_flock.h).
SRC=${1:-rl-cattle-herding_amd/csrc/ch_step.hip}
/opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC -ffp-contract=off --offload-arch=gfx950 -Iinclude ${EXTRA:-} \
  --cuda-device-only -c "$SRC" -o /tmp/res_usage.o -Rpass-analysis=kernel-resource-usage 2>&1 |
  grep -E "Function Name|VGPRs:|AGPRs|ScratchSize|Occupancy|SGPRs:" |
  sed -E 's/.*remark: //' | paste - - - - - - | grep -E "${FILTER:-k_step2}" | sed -E 's/\s+/ /g'
