#!/bin/bash
# round 4: suite + bench (default, with extras) + parity step profile + the forced-DP step profile (the same-box A/B
# of the split-weight picker went with its switch: profiles/r04 keeps the result)
R=${GRAFT_REPO_ROOT:-$(pwd)}; O=$R/gpurun_out/${TAG:-r4c}; mkdir -p $O; cd $R
TAG=${TAG:-r4c} bash tools/r4/gpu_suite.sh || exit $?
TAG=${TAG:-r4c}/prof PREC=bf16-parity bash tools/r4/gpu_prof.sh > /dev/null || exit $?
head -3 $O/prof/step.txt; cat $O/prof/phases.txt
MTTS_FORCE_DP=1 TAG=${TAG:-r4c}/prof_dp PREC=bf16-parity bash tools/r4/gpu_prof.sh > /dev/null || exit $?
head -3 $O/prof_dp/step.txt; cat $O/prof_dp/phases.txt
