// Sample i of the stream the Task-4 receiver works on, computed from the received frame on the fly with the roundings of the
// separate stages: the STO fix add_STO(rx, TgPosition), add_STO(., -(Nfft + T_guard)) (T4/Main_model_Task_4.m:292-294) as an index
// shift with zeros in front, and add_CFO(., cfo) (:301, remove_IFO.m:9) as one rotation rounded to T.  One definition for the
// receiver's direct form (ofdm_chain_t4.hip) and the integer-CFO capture (ofdm_ifo_study.hip).
#pragma once

#include "ofdm_common.hpp"

namespace ofdm {

template <typename T>
__device__ __forceinline__ cx<T> t4_raw(const cx<T>* __restrict__ x, int64_t i, int64_t len, int sym_len, int time_desync,
                                        int64_t pos) {
  if (!time_desync) return nt_load(x + i);
  const int64_t i1 = i - sym_len;
  return (i1 >= 0 && i1 < len - pos && i1 + pos < len) ? nt_load(x + i1 + pos) : mk<T>(0, 0);
}
template <typename T>
__device__ __forceinline__ cx<T> t4_rotate(cx<T> v, double cfo, int64_t i, double inv_nfft) {
  const double t = cfo * (double)i * inv_nfft;
  double sn, cs;
  sincospi(2.0 * (t - floor(t)), &sn, &cs);
  return mk<T>((T)((double)v.x * cs - (double)v.y * sn), (T)((double)v.x * sn + (double)v.y * cs));
}

}  // namespace ofdm
