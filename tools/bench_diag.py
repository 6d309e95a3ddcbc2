import ctypes as C, sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import __graft_entry__ as g
g.build()
from agp_amd import capi
L = capi.lib()
f = L.agp_dev_diag_bench
f.restype = C.c_int32
f.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_double)]
ctx = C.c_void_p()
assert L.agp_ctx_create(0, C.c_void_p(torch.cuda.current_stream().cuda_stream), C.byref(ctx)) == 0
names = {1: "2-level", 13: "2-level, no X21"}  # 1: k_chol_step / k_chol_safe ; 13: the chain of k_chol_dag (fp64 only)
failed = 0
for dt, dn in ((0, "f64"), (1, "f32")):
    for blocks in (1, 16):
        for v in ((1, 13) if dt == 0 else (1,)):
            us = C.c_double()
            rc = f(ctx, dt, v, blocks, 50, C.byref(us))
            if rc:
                failed += 1
                print(f"FAILED {dn} blocks={blocks:3d} {names[v]}: status {rc}")
                continue
            print(f"{dn} blocks={blocks:3d} {names[v]:42s} {us.value:8.2f} us/tile  ({us.value*2.1e3/64:6.0f} cyc/col @2.1GHz)")
L.agp_ctx_destroy(ctx)
sys.exit(1 if failed else 0)
