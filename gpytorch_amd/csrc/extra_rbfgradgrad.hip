// extern "C" entry points of the RBF kernel with first- and second-derivative observations (kv_rbfgradgrad.hpp: 2 d + 1 components per point): the
// fused product and its bilinear derivative.  Checks, plan and launches: kv_rbfgrad_host.hpp at derivative order 2.
#include "kv_rbfgrad_host.hpp"

using namespace gpamd;

extern "C" {

int gpamd_kv_rbfgradgrad_plan(int n, int m, int d, int t, int64_t ldo, int* S_host, int* jchunk_host, int64_t* workspace_floats_host) {
  return rgh::plan<2>("kv_rbfgradgrad_plan", n, m, d, t, ldo, S_host, jchunk_host, workspace_floats_host);
}

int gpamd_kv_rbfgradgrad_partials_f32(const float* inv_ls, int d, const float* X1p, int n, const float* X2p, int m, const float* Vt, int64_t ldv, int t,
                                      float* P, int64_t ldo, int S, int jchunk, const int* done, void* stream) {
  return rgh::partials<KRG_RBF, 2>("kv_rbfgradgrad", inv_ls, d, X1p, n, X2p, m, Vt, ldv, t, P, ldo, S, jchunk, done, stream);
}

int64_t gpamd_kv_rbfgradgrad_grad_workspace_doubles(int n, int m, int d) { return rgh::grad_workspace_doubles(n, m, d); }

int gpamd_kv_rbfgradgrad_grad_f32(const float* inv_ls, int d, const float* X1p, int n, const float* X2p, int m, const float* Lt, int64_t ldl,
                                  const float* Rt, int64_t ldr, int t, float* out, double* workspace, int64_t workspace_doubles, void* stream) {
  return rgh::grad<KRG_RBF, 2>("kv_rbfgradgrad_grad", inv_ls, d, X1p, n, X2p, m, Lt, ldl, Rt, ldr, t, out, workspace, workspace_doubles, stream);
}

}  // extern "C"
