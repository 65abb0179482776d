// Compile check for the direct lighting pass under its global name (host/ReferenceNames.h): a program written the way the
// reference's application entry point sets its passes (BidirectionalPathtracing/Main.cpp:9-29), here a G-buffer pass and
// LambertianPlusShadowPass::create() (CommonPasses/LambertianPlusShadowPass.h:31), must compile against the host mirror without
// any `using namespace`.  Written for this test; built with -fsyntax-only by tests/test_direct_cpu.py.
#include "ReferenceNames.h"

int main() {
  RenderingPipeline* pipeline = new RenderingPipeline();
  pipeline->setPass(0, LightProbeGBufferPass::create());
  pipeline->setPass(1, LambertianPlusShadowPass::create());
  LambertianPlusShadowPass::SharedPtr hinted = LambertianPlusShadowPass::create();
  hinted->setUseHints(true);
  RenderPass::SharedPtr asPass = hinted;
  SampleConfig config;
  config.windowDesc.resizableWindow = true;
  config.windowDesc.width = 1280;
  config.windowDesc.height = 720;
  config.windowDesc.title = "compile check";
  RenderingPipeline::run(pipeline, config);
  return asPass->getName() == "Lambertian Plus Shadows" ? 0 : 1;
}
