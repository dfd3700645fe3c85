#!/bin/bash
# Rebuilds the library with cycle stamps in the Jacobi tick kernels (GPU box, scratch copy only) and prints the per-launch
# phase times of jacobi_tick3_kernel: N = 160 and 192 (rows of 256, the Rayleigh-Ritz shape) and N = 500 (rows of 512).
# One process per size: the stamp slots add up over the life of a process.
ROOT=$(cd "$(dirname "$0")/.." && pwd)
cd $ROOT/dnn-compression-tensor-admm_amd/csrc && touch jacobi.hip plan.hip && make CXXEXTRA=-DTADMM_STAMPS > /dev/null 2>&1
cd $ROOT
for N in 160 192 500; do
TADMM_STAMPS_DUMP=1 python3 - $N <<'PY'
import sys
sys.path.insert(0, "dnn-compression-tensor-admm_amd")
import torch
from tadmm import ops
N = int(sys.argv[1])
torch.manual_seed(0)
a = torch.randn(N, 4 * N, dtype=torch.float64, device="cuda")
g = a @ a.T
ev, vec, sweeps = ops.eigh(g)
print("N", N, "sweeps", sweeps, file=sys.stderr)
PY
done
