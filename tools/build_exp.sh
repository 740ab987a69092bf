#!/bin/bash
# developer tool: experiment build of libsc_engine.so (-DSC_EXP knobs) into smart-chess-rust_amd/lib_exp/
set -e
R=$(cd $(dirname $0)/.. && pwd)
C=$R/smart-chess-rust_amd/csrc; O=$R/smart-chess-rust_amd/lib_exp$SC_EXP_TAG; mkdir -p $O
H="/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -DSC_EXP $SC_EXP_DEFS"
$H -ffp-contract=off -c $C/mcts_kernels.hip -o $O/mcts.o 
$H -ffp-contract=off -c $C/encode_kernels.hip -o $O/encode.o
$H -mllvm -amdgpu-mfma-vgpr-form=1 -c $C/nn_kernels.hip -o $O/nn.o 
$H -mllvm -amdgpu-mfma-vgpr-form=1 -c $C/step_kernels.hip -o $O/step.o
$H -ffp-contract=off -c $C/score_kernels.hip -o $O/score.o
$H -c $C/batch_kernels.hip -o $O/batch.o
for u in engine encode_steps device_calls selfplay selfplay_io; do $H -c $C/$u.hip -o $O/$u.o; done   # the host layer
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o $O/libsc_engine.so $O/*.o -Wl,-rpath,/opt/rocm/lib
rm -f $O/*.o; ls -la $O
