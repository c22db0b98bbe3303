// Times one application of the harness operator (Ipm::kmult: the Hessian product of a QP handle, then the two block-angular products
// with their epilogues) with HIP events, on a handle made through the C ABI.  The harness is a single translation unit, so this probe
// includes it to see the handle's layout; it is built by tools/qp_operator_probe.py and loaded beside libpipship.so, whose own
// entries made the handle.  Not part of the library.
// The cast below is valid only while this file is compiled with the flags of csrc/Makefile (tools/qp_operator_probe.py passes the same
// ones and rebuilds when harness.hip is newer): the layout of pips::Ipm must be the library's.  This .so also carries copies of the
// harness' kernels and extern "C" entries; libpipship.so is loaded first with RTLD_GLOBAL, so the library's entries are the ones bound.
#include "../pips-ipmpp_amd/csrc/harness.hip"

extern "C" int qp_probe_kmult(void* handle, int warmup, int reps, float* ms_out, long long* dims3) {
   pips::Ipm* p = (pips::Ipm*)handle;
   if (!p || reps < 1 || !ms_out) return 1;
   if (hipSetDevice(p->device) != hipSuccess) return 2;
   if (pips_hip_vec_set(p->nxyz, 1.0, p->w_dx, p->stream)) return 3;
   hipEvent_t e0, e1;
   if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) return 4;
   int rc = 0;
   for (int k = 0; k < warmup + reps && !rc; ++k) {
      (void)hipEventRecord(e0, p->stream);
      rc = p->kmult(p->w_dx, p->w_v);
      (void)hipEventRecord(e1, p->stream);
      if (hipEventSynchronize(e1) != hipSuccess) rc = 5;
      float ms = 0.f;
      (void)hipEventElapsedTime(&ms, e0, e1);
      if (k >= warmup) ms_out[k - warmup] = ms;
   }
   if (dims3) { dims3[0] = p->nxyz; dims3[1] = p->J_nnz; dims3[2] = p->has_q ? p->Q_nnz : 0; }
   (void)hipEventDestroy(e0);
   (void)hipEventDestroy(e1);
   return rc;
}
