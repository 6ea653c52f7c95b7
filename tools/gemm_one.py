"""Run one GEMM shape/variant repeatedly (for PMC collection)."""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from aware_amd import runtime as rt
M, N, K, v, reps = [int(x) for x in sys.argv[1:6]]
a = torch.randn(M, K, device="cuda"); b = torch.randn(N, K, device="cuda"); c = torch.empty(M, N, device="cuda")
for _ in range(reps):
    rt.gemm_nt_variant(a, b, None, v, out=c)
torch.cuda.synchronize()
