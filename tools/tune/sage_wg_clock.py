"""Measurement-only variant of csrc/wg_sage_mfma.hip: every workgroup of sage_layer_mfma_kernel leaves its begin and end time
(wall_clock64, 100 MHz) in a device array that `wgamd_dbg_wg_clock` copies out and clears.  The shipped kernel carries no such
code; this script writes a patched COPY of the source, to be compiled in place of the original into a library of its own:

    python tools/tune/sage_wg_clock.py cugraph-gnn_amd/csrc/wg_sage_mfma.hip build_tune/wg_clock/wg_sage_mfma.hip
    hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -fno-gpu-rdc -Iinclude -Icugraph-gnn_amd/csrc -c build_tune/wg_clock/wg_sage_mfma.hip -o build_tune/wg_clock/wg_sage_mfma.o
    hipcc --offload-arch=gfx950 -shared -fPIC -o build_tune/wg_clock/libwholegraph_amd.so <the library's other objects> build_tune/wg_clock/wg_sage_mfma.o -ldl
    WGAMD_LIBRARY_PATH=build_tune/wg_clock/libwholegraph_amd.so python tools/profile_sage_tile_tail.py

(profiles/r07/README.md has the numbers this produced.)"""
import sys
src, dst = sys.argv[1], sys.argv[2]
s = open(src).read()
s = s.replace('#include "wg_sage_mfma_parts.hpp"\n', '#include "wg_sage_mfma_parts.hpp"\n__device__ unsigned long long g_wg_clock[2][1024];\n', 1)
old = '''  extern __shared__ __attribute__((aligned(16))) float lds[];
'''
assert s.count(old) == 1
s = s.replace(old, old + '  if (threadIdx.x == 0) g_wg_clock[0][blockIdx.x] = wall_clock64();\n')
# end of the kernel: every wave's lane 0 -> max
if 'atomicAdd(a.tickets + 1, 1u)' in s:
    old = '''  // Every ticket this workgroup drew came back'''
else:
    old = '''}

// ---- weight in the order the multiplying waves read it'''
assert s.count(old) == 1
s = s.replace(old, '  if ((threadIdx.x & 63) == 0) atomicMax(&g_wg_clock[1][blockIdx.x], (unsigned long long)wall_clock64());\n' + old)
s += '''
extern "C" int wgamd_dbg_wg_clock(unsigned long long* out)
{
  if (hipDeviceSynchronize() != hipSuccess) return 1;
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_wg_clock), sizeof(g_wg_clock)) != hipSuccess) return 2;
  static unsigned long long zeros[2][1024];
  if (hipMemcpyToSymbol(HIP_SYMBOL(g_wg_clock), zeros, sizeof(zeros)) != hipSuccess) return 3;
  return 0;
}
'''
open(dst, 'w').write(s)
