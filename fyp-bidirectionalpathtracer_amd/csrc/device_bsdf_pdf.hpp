// device_bsdf_pdf.hpp — the BSDF toward a given direction as multiple importance sampling needs it: the unweighted
// BSDF times cosine of next-event estimation, and the solid-angle density with which sampleBRDF draws that direction
// (include/bdpt.h "Environment lighting", bdpt_bsdf_pdf_query).  One text for the dense query kernel (env_light.hip) and
// the fused pass (sky_mis.hip); every term is a function of device_math.hpp, in fp32 as written.
#pragma once
#include "device_math.hpp"

namespace bdpt {

// Lambertian: fcos = (NdotL * dif) / kPi and sampleBRDF<false>'s own pdf expression.
// GGX: fcos = directIfVisible<true> with one light of intensity 1 (D G F / (4 NdotV) + NdotL dif / kPi); pdf = the
// one-sample mixture of sampleBRDF<true>'s two lobes, chosen with probabilityToSampleDiffuse, and 0 when dot(N, L) <= 0,
// where both lobes refuse the direction.
template <bool GGX>
__device__ __forceinline__ void bsdfFcosPdf(f3 L, f3 N, f3 V, f3 dif, f3 spec, float rough, f3& fcos, float& pdf) {
  if (GGX) {
    fcos = directIfVisible<true>(1.0f, L, mk(1.0f), N, V, dif, spec, rough);
    pdf = 0.0f;
    if (!(dot(N, L) <= 0.0f)) {
      const float NdotL = saturate(dot(N, L));
      const float pd = probabilityToSampleDiffuse(dif, spec);
      const float pdfD = (NdotL * kInvPi) * pd;
      const f3 H = normalize(V + L);
      const float NdotH = saturate(dot(N, H));
      const float LdotH = saturate(dot(L, H));
      const float pdfS = (ggxNormalDistribution(NdotH, rough) * NdotH / (4 * LdotH)) * (1.0f - pd);
      pdf = pdfD + pdfS;
    }
  } else {
    const float NdotL = saturate(dot(N, L));
    fcos = (NdotL * dif) / kPi;
    pdf = NdotL * kInvPi;
  }
}

}  // namespace bdpt
