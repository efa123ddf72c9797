// The activations of GraphGym's act_dict (graphgym/models/act.py:6-14) and SiLU, written once: act_fwd<ACT> and
// act_grad<ACT> on the fp32 pre-activation z, for every pass of bn.hip that applies or differentiates one.  ACT is a
// template parameter (MP_ACT_* of include/mp_engine.h): a kind costs the others nothing.  `p` is the kind's parameter:
// the negative slope of LRELU / PRELU (PRELU's is read from the device by the kernel and handed in), ELU's alpha.
#pragma once
#include <hip/hip_runtime.h>
#include <type_traits>
#include "../../include/mp_engine.h"

namespace mp {

// torch.nn.SELU's two constants (torch/nn/modules/activation.py, aten/src/ATen/native/Activation.cpp)
constexpr float kSeluAlpha = 1.6732632423543772848170429916717f;
constexpr float kSeluScale = 1.0507009873554804934193349852946f;

template <int ACT>
__device__ __forceinline__ float act_fwd(float z, float p) {
  if constexpr (ACT == MP_ACT_RELU) return z > 0.f ? z : 0.f;
  else if constexpr (ACT == MP_ACT_LRELU || ACT == MP_ACT_PRELU) return z > 0.f ? z : p * z;
  else if constexpr (ACT == MP_ACT_ELU) return z > 0.f ? z : p * expm1f(z);
  else if constexpr (ACT == MP_ACT_SELU) return kSeluScale * (z > 0.f ? z : kSeluAlpha * expm1f(z));
  else if constexpr (ACT == MP_ACT_SILU) return z / (1.f + expf(-z));
  else return z;
}

// d act / d z
template <int ACT>
__device__ __forceinline__ float act_grad(float z, float p) {
  if constexpr (ACT == MP_ACT_RELU) return z > 0.f ? 1.f : 0.f;
  else if constexpr (ACT == MP_ACT_LRELU || ACT == MP_ACT_PRELU) return z > 0.f ? 1.f : p;
  else if constexpr (ACT == MP_ACT_ELU) return z > 0.f ? 1.f : p * expf(z);
  else if constexpr (ACT == MP_ACT_SELU) return kSeluScale * (z > 0.f ? 1.f : kSeluAlpha * expf(z));
  else if constexpr (ACT == MP_ACT_SILU) {
    const float s = 1.f / (1.f + expf(-z));
    return s * (1.f + z * (1.f - s));
  } else return 1.f;
}

// g = dy * act'(z).  RELU selects (a masked element is +0 whatever dy's sign: the bits of the ReLU backward that reads
// the forward's output); the others multiply.
template <int ACT>
__device__ __forceinline__ float act_bwd(float dy, float z, float p) {
  if constexpr (ACT == MP_ACT_RELU) return z > 0.f ? dy : 0.f;
  else if constexpr (ACT == MP_ACT_LRELU || ACT == MP_ACT_PRELU) return z > 0.f ? dy : p * dy;
  else return dy * act_grad<ACT>(z, p);
}

// PRELU: d act / d slope
__device__ __forceinline__ float act_dslope(float z) { return z > 0.f ? 0.f : z; }

// runtime kind -> template argument: f receives std::integral_constant<int, MP_ACT_*>; false for a kind that is not
// MP_ACT_NONE or one of the six activations
template <class Fn>
static inline bool with_act(int act, Fn&& f) {
  switch (act) {
    case MP_ACT_NONE: f(std::integral_constant<int, MP_ACT_NONE>{}); return true;
    case MP_ACT_RELU: f(std::integral_constant<int, MP_ACT_RELU>{}); return true;
    case MP_ACT_LRELU: f(std::integral_constant<int, MP_ACT_LRELU>{}); return true;
    case MP_ACT_PRELU: f(std::integral_constant<int, MP_ACT_PRELU>{}); return true;
    case MP_ACT_ELU: f(std::integral_constant<int, MP_ACT_ELU>{}); return true;
    case MP_ACT_SELU: f(std::integral_constant<int, MP_ACT_SELU>{}); return true;
    case MP_ACT_SILU: f(std::integral_constant<int, MP_ACT_SILU>{}); return true;
    default: return false;
  }
}

}  // namespace mp
