#!/bin/bash
# where a k-tile of the bf16-split GEMM (csrc/gemm_split_bf16.inc, in both library variants) spends its time: diagnostic builds
# (results are garbage in them; built as the experimental variant so that the shipped library stays as it is), microbenchmark
# of the F/A-like and the D launch shapes with SET_GEMM_SPLIT=1.  tools/split_diag.sh
cd $GRAFT_REPO_ROOT
export SET_LIB_VARIANT=exp SET_GEMM_SPLIT=1 ITERS=100
for f in "" "-DSPL_EXP_NOSPLIT" "-DSPL_EXP_NOMFMA" "-DSPL_EXP_NOGLOAD" "-DSPL_EXP_NOSPLIT -DSPL_EXP_NOGLOAD" "-DSPL_EXP_NOSPLIT -DSPL_EXP_NOMFMA -DSPL_EXP_NOGLOAD"; do
  SET_HIPCC_FLAGS="$f" python -m show_edit_tell_amd.build --exp --force > /dev/null 2>&1
  echo "== [$f]"
  python tools/gemm_microbench.py 128 18192 1024 128 4096 3072 2>&1 | grep -v amdgpu.ids
done
python -m show_edit_tell_amd.build --exp --force > /dev/null 2>&1
