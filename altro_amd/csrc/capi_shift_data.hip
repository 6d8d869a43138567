// capi_shift_data.hip -- C ABI: the problem DATA of a receding-horizon step, moved and rewritten in place: dynamics given as data
// (altro_hip_set_dynamics_range / _get_dynamics_knot / _shift_dynamics) and the cost's linear terms (altro_hip_shift_linear_costs).
// shift_fields.h says where they live on each plan; kernels/shift_field.hip moves them; the setters' own packers write a range.
#include "capi_internal.h"

#include <vector>

using namespace altro_hip;
using namespace altro_hip::capi;

namespace {

// the handles the dynamics-as-data calls refuse, after check(h)
int dyn_data_entry(altro_hip_batch* h, const char* call) {
  if (h->ragged) return fail(ALTRO_HIP_ERR_UNSUPPORTED, "%s needs uniform dimensions (the handle has per-knot-point dimensions)", call);
  if (h->model_set)
    return fail(ALTRO_HIP_ERR_NOT_SET, "%s: the handle has a device model -- its dynamics are the model's (altro_hip_set_time_steps moves its grid)", call);
  if (h->host_batch > 0)
    return fail(ALTRO_HIP_ERR_UNSUPPORTED, "%s: altro_hip_set_host_batch is in effect -- a staging aid for synthetic batches, not an MPC path", call);
  if (!h->dyn_set) return fail(ALTRO_HIP_ERR_NOT_SET, "%s: altro_hip_set_dynamics has not been called", call);
  return 0;
}

// the getter hands out HOST arrays in either pointer mode
struct HostPointers {
  altro_hip_batch* h;
  bool was;
  explicit HostPointers(altro_hip_batch* h_) : h(h_), was(h_->dev_ptrs) { h->dev_ptrs = false; }
  ~HostPointers() { h->dev_ptrs = was; }
};

// every field of `fields` one knot point forward over K knot points (kernels/shift_field.hip), on the handle's stream
int shift_fields_run(altro_hip_batch* h, const FieldRef* fields, int count, int K, const char* what) {
  for (int i = 0; i < count; ++i) {
    const ShiftRun r = shift_run(fields[i], h->batch, K, (int)h->esz);
    const int rc = shift_field_launch(h->stream, loop_buffer(h, fields[i].buf), (int)h->esz, r);
    if (rc == 1) return fail(ALTRO_HIP_ERR_UNSUPPORTED, "%s: field %d cannot be walked in place (run %lld, knot-point stride %lld)", what, i, (long long)r.run, (long long)r.ks);
    if (rc) return fail(ALTRO_HIP_ERR_HIP, "%s: shift kernel launch failed", what);
  }
  return 0;
}

}  // namespace

extern "C" {

int altro_hip_set_dynamics_range(altro_hip_batch* h, const double* A, const double* B, const double* f, int k_first, int k_last, int bz) {
  int rc = check(h);
  if (rc) return rc;
  const int n = h->n, m = h->m, N = h->N;
  if (k_first < 0 || k_last > N - 1 || k_first > k_last)
    return fail(ALTRO_HIP_ERR_BAD_ARGUMENT, "knot point range [%d, %d] outside [0, %d]", k_first, k_last, N - 1);
  if (!A || !B) return fail(ALTRO_HIP_ERR_BAD_ARGUMENT, "A and B are required");
  if ((rc = dyn_data_entry(h, "altro_hip_set_dynamics_range"))) return rc;
  h->expansion_current = false; h->aff_base = false;
  const int nk = k_last - k_first + 1;
  if (h->plan == ALTRO_HIP_PLAN_MFMA16) {
    DevSrc dA, dB, df;
    rc = put_src(h, A, n * n, nk, 0, bz, &dA);
    if (!rc) rc = put_src(h, B, n * m, nk, 0, bz, &dB);
    if (!rc) rc = put_src(h, f, n, nk, 0, bz, &df);
    if (!rc) rc = mfma16_pack_launch(h, MSEG_Z, dA.s, dB.s, nullptr, nullptr, -1, k_first, nk);
    if (!rc) rc = mfma16_pack_launch(h, MSEG_F, df.s, SrcArr{nullptr, 0, 0, 0}, nullptr, nullptr, -1, k_first, nk);
    if (!rc) HIP_TRY(hipStreamSynchronize(h->stream));   // (before the sources' temporaries go)
  } else if (h->plan == ALTRO_HIP_PLAN_LANE) {
    const LaneSizes z = lane_sizes(n, m);
    auto pk = [&](const double* src, int len, int off) -> int {
      return lane_pack(h, h->l_in, (int64_t)k_first * z.e_in * h->batch, z.e_in, src, len, off, 0, nk, 0, nk, 0, bz);
    };
    rc = pk(A, n * n, 0);
    if (!rc) rc = pk(B, n * m, n * n);
    if (!rc) rc = pk(f, n, n * n + n * m);
  } else {
    rc = generic_set(h, G_A, A, n * n, nk, 0, bz, k_first);
    if (!rc) rc = generic_set(h, G_B, B, n * m, nk, 0, bz, k_first);
    if (!rc) {
      if (f) rc = generic_set(h, G_f, f, n, nk, 0, bz, k_first);
      else   // the range's rows of [b][k][n]: nk * n elements of every problem's N * n
        HIP_TRY(hipMemset2DAsync((char*)h->g_arr[G_f] + (size_t)k_first * n * h->esz, (size_t)h->g_bstride[G_f] * h->esz, 0, (size_t)nk * n * h->esz, h->batch, h->stream));
    }
  }
  if (rc) return rc;
  HIP_TRY(hipStreamSynchronize(h->stream));
  if (f) h->has_f = 1;
  return 0;
}

int altro_hip_get_dynamics_knot(altro_hip_batch* h, int k, double* A, double* B, double* f) {
  int rc = check(h);
  if (rc) return rc;
  const int n = h->n, m = h->m, N = h->N;
  if (k < 0 || k > N - 1) return fail(ALTRO_HIP_ERR_BAD_ARGUMENT, "knot point %d outside [0, %d]", k, N - 1);
  if ((rc = dyn_data_entry(h, "altro_hip_get_dynamics_knot"))) return rc;
  HostPointers host(h);
  if (h->plan == ALTRO_HIP_PLAN_MFMA16) {   // Z = [A B] as altro_hip_get_expansion reads it; f is the head of the record's f slot
    if ((A || B) && (rc = mfma16_get_z(h, k, 1, A, B))) return rc;
    if (f) rc = aos_get(h, f, h->m_in, k * h->m_st.in_ks + MF_OFF_F, h->m_st.in_bs, h->m_st.in_ks, n, 1);
    return rc;
  }
  FieldRef fr[3];
  const int count = dyn_fields(dyn_shape(h), k, fr);
  double* const dst[3] = {A, B, f};
  const int len[3] = {n * n, n * m, n};
  if (count == 1) {   // plan LANE: A | B | f back to back in the record
    int off = (int)fr[0].off;
    for (int i = 0; i < 3 && !rc; off += len[i], ++i)
      if (dst[i]) rc = lane_get(h, dst[i], loop_buffer(h, fr[0].buf), (int64_t)k * fr[0].ks, nullptr, fr[0].E, off, 0, len[i], 1, 1);
    return rc;
  }
  for (int i = 0; i < count && !rc; ++i)
    if (dst[i]) rc = aos_get(h, dst[i], loop_buffer(h, fr[i].buf), fr[i].off, fr[i].bs, fr[i].ks, fr[i].len, 1);
  return rc;
}

int altro_hip_shift_dynamics(altro_hip_batch* h) {
  int rc = check(h);
  if (rc) return rc;
  if ((rc = dyn_data_entry(h, "altro_hip_shift_dynamics"))) return rc;
  h->expansion_current = false; h->aff_base = false;
  FieldRef fr[3];
  const int count = dyn_fields(dyn_shape(h), 0, fr);
  return shift_fields_run(h, fr, count, h->N, "altro_hip_shift_dynamics");
}

int altro_hip_shift_linear_costs(altro_hip_batch* h) {
  int rc = loop_entry(h, true);
  if (rc) return rc;
  if (h->ragged) return fail(ALTRO_HIP_ERR_UNSUPPORTED, "altro_hip_shift_linear_costs needs uniform dimensions");
  if (!h->lqr_cost_set) return fail(ALTRO_HIP_ERR_NOT_SET, "no quadratic cost to shift (ErrorCodes::CostNotQuadratic)");
  h->expansion_current = false;
  FieldRef fr[3];
  const int count = linear_cost_fields(loop_shape(h), fr);
  return shift_fields_run(h, fr, count, h->N, "altro_hip_shift_linear_costs");
}

}  // extern "C"
