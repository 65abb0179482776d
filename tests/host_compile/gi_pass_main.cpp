// Compile check for the diffuse GI pass under its global name (host/ReferenceNames.h): a program written the way the
// reference's application entry point sets its passes (BidirectionalPathtracing/Main.cpp:9-29), here a G-buffer pass,
// SimpleDiffuseGIPass::create(channel) (CommonPasses/SimpleDiffuseGIPass.h:32) and the accumulation pass, must compile against
// the host mirror without any `using namespace`.  Written for this test; built with -fsyntax-only by tests/test_gi_cpu.py.
#include "ReferenceNames.h"

int main() {
  RenderingPipeline* pipeline = new RenderingPipeline();
  pipeline->setPass(0, LightProbeGBufferPass::create());
  pipeline->setPass(1, SimpleDiffuseGIPass::create(ResourceManager::kOutputChannel));
  pipeline->setPass(2, SimpleAccumulationPass::create(ResourceManager::kOutputChannel));
  SimpleDiffuseGIPass::SharedPtr toChannel = SimpleDiffuseGIPass::create("DiffuseGI");
  RenderPass::SharedPtr asPass = toChannel;
  SampleConfig config;
  config.windowDesc.resizableWindow = true;
  config.windowDesc.width = 1280;
  config.windowDesc.height = 720;
  config.windowDesc.title = "compile check";
  RenderingPipeline::run(pipeline, config);
  return asPass->getName() == "Simple Diffuse GI Ray" ? 0 : 1;
}
