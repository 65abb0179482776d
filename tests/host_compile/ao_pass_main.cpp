// Compile check for the ambient occlusion pass under its global name (host/ReferenceNames.h): a program written the way
// the reference's application entry point sets its passes (BidirectionalPathtracing/Main.cpp:9-29), here a G-buffer pass
// and AmbientOcclusionPass::create(channel) (CommonPasses/AmbientOcclusionPass.h:32), must compile against the host mirror without any
// `using namespace`.  Written for this test; built with -fsyntax-only by tests/test_ao_cpu.py.
#include "ReferenceNames.h"

int main() {
  RenderingPipeline* pipeline = new RenderingPipeline();
  pipeline->setPass(0, LightProbeGBufferPass::create());
  pipeline->setPass(1, AmbientOcclusionPass::create(ResourceManager::kOutputChannel));
  AmbientOcclusionPass::SharedPtr toOutput = AmbientOcclusionPass::create();  // the default channel is the pipeline's output
  RenderPass::SharedPtr asPass = toOutput;
  SampleConfig config;
  config.windowDesc.resizableWindow = true;
  config.windowDesc.width = 1280;
  config.windowDesc.height = 720;
  config.windowDesc.title = "compile check";
  RenderingPipeline::run(pipeline, config);
  return asPass->getName() == "Ambient Occlusion Rays" ? 0 : 1;
}
