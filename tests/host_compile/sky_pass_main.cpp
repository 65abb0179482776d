// Compile check for the sky lighting pass under its global name (host/ReferenceNames.h): a program written the way the
// reference's application entry point sets its passes (BidirectionalPathtracing/Main.cpp:9-29), here a G-buffer pass,
// SkyLightingPass::create(channel) and the accumulation pass, must compile against the host mirror without any
// `using namespace`.  Written for this test; built with -fsyntax-only by tests/test_env_cpu.py.
#include "ReferenceNames.h"

int main() {
  RenderingPipeline* pipeline = new RenderingPipeline();
  pipeline->setPass(0, LightProbeGBufferPass::create());
  SkyLightingPass::SharedPtr sky = SkyLightingPass::create(ResourceManager::kOutputChannel);
  sky->setClamp(4.0f);
  pipeline->setPass(1, sky);
  pipeline->setPass(2, SimpleAccumulationPass::create(ResourceManager::kOutputChannel));
  SkyLightingPass::SharedPtr toOutput = SkyLightingPass::create();  // the default channel is the pipeline's output
  RenderPass::SharedPtr asPass = toOutput;
  SampleConfig config;
  config.windowDesc.resizableWindow = true;
  config.windowDesc.width = 1280;
  config.windowDesc.height = 720;
  config.windowDesc.title = "compile check";
  RenderingPipeline::run(pipeline, config);
  return asPass->getName() == "Sky Lighting Rays" ? 0 : 1;
}
