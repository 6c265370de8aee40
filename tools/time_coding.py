import sys, time, torch
sys.path.insert(0, "/root/repo")
from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd.graphs.models.LiftingBasedDWT_net import LiftingBasedDWTNetWrapper
from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd.utils.config import make_config
for ent in ("conditioned2ZTsepSubbands", "onlyEZWT", "DWTConditioned2EntropyLayerZTBlock"):
    cfg = make_config(dwtlevels=4, mode="validate", entropy_layer=ent)
    torch.manual_seed(0)
    net = LiftingBasedDWTNetWrapper(cfg).to("cuda:0").eval()
    x = torch.rand(1, 3, 512, 512, device="cuda:0")
    with torch.no_grad():
        net.compress(x[:, :, :64, :64])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        xhat, bxe, bxo = net.compress(x)
        torch.cuda.synchronize()
        print(ent, "compress+decompress of one 3x512x512 image: %.2f s, %.3f bpp" % (time.perf_counter() - t0, float(bxe + bxo)))
