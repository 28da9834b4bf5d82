#!/bin/bash
# 300^3 CG + GAMG with three level smoothers, one process per solve, in one job
# on one box: Richardson(1) (configs/cg_gamg.info), Chebyshev(1)
# (configs/cg_gamg_cheby.info) and Chebyshev(2), each twice in a row (the
# second is the one quoted), then Richardson(1) and Chebyshev(1) once more.
#   profiles/mg_smoothers/run.sh [output directory]      (from the repository root)
set -o pipefail
out=${1:-out/mg_smoothers_300}
mkdir -p $out
exe=petsc-openacc_amd/bin/main_ksp
grid="-da_grid_x 300 -da_grid_y 300 -da_grid_z 300 -aijhip_iteration_bytes"
run() { timeout -k 10 120 $exe $2 $grid > $out/$1.txt 2> $out/$1.err; }
(rocm-smi --showproductname 2>/dev/null | head -12; echo GPU_MAX_HW_QUEUES=$GPU_MAX_HW_QUEUES) > $out/box.txt
run richardson1_run1 "-config configs/cg_gamg.info" && run richardson1_run2 "-config configs/cg_gamg.info" &&
run chebyshev1_run1 "-config configs/cg_gamg_cheby.info" && run chebyshev1_run2 "-config configs/cg_gamg_cheby.info" &&
run chebyshev2_run1 "-config configs/cg_gamg_cheby.info -aijhip_mg_levels_ksp_max_it 2" &&
run chebyshev2_run2 "-config configs/cg_gamg_cheby.info -aijhip_mg_levels_ksp_max_it 2" &&
run richardson1_run3 "-config configs/cg_gamg.info" && run chebyshev1_run3 "-config configs/cg_gamg_cheby.info"
rc=$?
tail -n 7 $out/*.txt
cat $out/*.err | head -20
exit $rc
