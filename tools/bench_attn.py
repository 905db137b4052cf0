#!/usr/bin/env python3
"""Timing of attention32_kernel at Register shape (B=252 T=400; env B, T, V): variant 1 = as shipped, 8 = without its XCD remap, 16 + x = the timing
ablations (wrong results; the ids are the rows of ATT_VARIANTS in fp_nn.hip, e.g. 17 no staging, 18 no softmax, 20 no PV, 24 no QK, 30 staging only)."""
import ctypes, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from foundationpose_cpp_amd import _lib
_lib.use_test_lib()
L = _lib.lib()
L.fpt_attention_bench.restype = ctypes.c_float
L.fpt_attention_bench.argtypes = [ctypes.c_int] * 4
B, T = int(os.environ.get("B", 252)), int(os.environ.get("T", 400))
for v in [int(x) for x in os.environ.get('V', '1,8').split(',')]:
    ms = L.fpt_attention_bench(B, T, 20, v)
    fl = 4.0 * B * 4 * T * T * 128
    print(f"variant {v}: {ms*1e3:8.1f} us  {fl/ms/1e9:7.1f} TF/s")
