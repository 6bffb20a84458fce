"""ResNet-50 without a GPU: the model's size and state_dict, the pointwise plans' invariants
(csrc/kernels/conv_pw.hip conv_pw_plan / conv_pw_wgrad_plan take sizes, no device), and one
train / save / resume run of the CLI on the CPU path."""
import os

import pytest
import torch

from ddp_amd import native
from ddp_amd.models import resnet18, resnet50

CHANNELS = (64, 128, 192, 256, 512, 1024, 2048)


def test_resnet50_size_and_state_dict():
    m = resnet50()
    assert sum(p.numel() for p in m.parameters()) == 25_557_032
    sd = m.state_dict()
    assert tuple(sd["layer1.0.downsample.0.weight"].shape) == (256, 64, 1, 1)
    assert tuple(sd["layer4.2.conv3.weight"].shape) == (2048, 512, 1, 1)
    assert tuple(sd["fc.weight"].shape) == (1000, 2048)
    assert [len(getattr(m, f"layer{i}")) for i in range(1, 5)] == [3, 4, 6, 3]
    other = resnet50()
    other.load_state_dict(sd)
    assert all(torch.equal(v, other.state_dict()[k]) for k, v in sd.items())
    assert tuple(resnet18().state_dict()["fc.weight"].shape) == (1000, 512)  # (unchanged)


@pytest.mark.parametrize("Cout", CHANNELS)
def test_pointwise_plan_invariants(Cout):
    C = native.require()
    for P in range(1, 301):
        ok, bp, bc, rows = C.conv_pw_plan(P, 64, Cout)
        assert ok and (bp, bc) in ((128, 128), (128, 64), (64, 64)) and Cout % bc == 0
        assert rows == -(-P // bp)  # the grid covers the pixels, and one stats row per pixel tile
        for Cin in CHANNELS:
            bm, bn, ppc, chunks = C.conv_pw_wgrad_plan(P, Cin, Cout)
            assert Cout % bm == 0 and Cin % bn == 0 and ppc % 64 == 0
            assert (chunks - 1) * ppc < P <= chunks * ppc and chunks * Cout * Cin * 4 <= 16 << 20
    assert not C.conv_pw_plan(70, 96, Cout)[0] and not C.conv_pw_plan(70, Cout, 2112)[0]
    assert C.conv_pw_plan(70, 64, Cout, 128, 128)[0] == (Cout % 128 == 0)  # a forced tile must divide Cout
    assert bool(C.conv_pw_wgrad_plan(70, 192, Cout, 128, 128)[0]) is False  # ... and Cin
    assert C.conv_pw_plan(25088, 512, 256)[1:3] == (128, 128)  # long K, big grid: operand reuse ...
    assert C.conv_pw_plan(1568, 2048, 512)[1:] == (64, 64, 25)  # ... layer 4 takes the most blocks there are ...
    assert C.conv_pw_plan(100352, 64, 256)[1:3] == (64, 64)  # ... and a short K loop the most resident blocks
    assert C.conv_pw_wgrad_plan(1568, 512, 2048)[3] == 1 and C.conv_pw_wgrad_plan(100352, 64, 256)[3] > 100


def test_cli_trains_saves_and_resumes_resnet50(tmp_path, capfd):
    import train_ddp

    args = ["--model", "resnet50", "--device", "cpu", "--image_size", "32", "--num_classes", "8",
            "--dataset_size", "16", "--batch_size", "8", "--world_size", "1", "--checkpoint_dir", str(tmp_path)]
    train_ddp.main(args + ["--epochs", "1"])
    assert os.path.exists(tmp_path / "epoch_0.pt")
    train_ddp.main(args + ["--epochs", "2"])
    out = capfd.readouterr().out.lower()
    assert "resum" in out and os.path.exists(tmp_path / "epoch_1.pt")
