"""``JointSamTrainer`` on the device: two iterations on one 256 x 256 image with a Voronoi label image (synthetic vit_b, image encoder
frozen so that the test stays within seconds; mask decoder and UNETR decoder train).  Which parameters move in which of the two
optimisation passes, two optimizer steps per iteration, the same loss records from one-channel labels (targets made by the trainer on the
device) and from the four-channel layout, and the checkpoint through ``instance_segmentation.get_predictor_and_decoder``: the loaded
decoder on the image's embedding against the trainer's own UNETR (``np.allclose(atol=1e-4)``, the comparison of the HIP decoder with the
module's operator path in tests/test_gpu_ais.py).

The UNETR half is torch operators.  On the library (MIOpen) convolutions the first backward pass of a process compiles their kernels - 85 s
on a fresh machine - and their gradients, like those of the bilinear up-samplers, differ in the last bits from run to run,
so the instance loss of the SECOND iteration would not repeat.  The test is about the trainer, not about those operators: it runs the
convolutions on torch's own GEMM path (``torch.backends.cudnn.flags(enabled=False)``) and builds the decoder with transposed-convolution
up-samplers, which makes both halves repeat bit for bit, so that the records of the two label layouts can be compared for equality."""
import random

import numpy as np
import pytest
import torch

import labelprops_ref as LR

pytestmark = pytest.mark.gpu
ITERATIONS = 2


def _data():
    labels = LR.voronoi(256, 256, 12, 4)
    rng = np.random.default_rng(0)
    image = np.clip(40 + 15 * (labels % 5) * (labels > 0) + rng.normal(0, 6, labels.shape), 0, 255).astype(np.uint8)
    x = torch.as_tensor(image, dtype=torch.float32)[None, None].repeat(1, 3, 1, 1)
    return image, x, torch.as_tensor(labels.astype(np.int64))[None, None]


def _run(sd, x, y):
    """Two iterations from fixed seeds -> (trainer, the parameter snapshots after every optimizer step, the initial snapshot)."""
    from micro_sam_amd import util
    from micro_sam_amd.models import unetr as U
    from micro_sam_amd.training import ConvertToSamInputs, JointSamTrainer, TrainableSAM
    np.random.seed(3); random.seed(3); torch.manual_seed(3)
    predictor = util.get_sam_model("vit_b", device="cuda", state_dict=sd)
    model = TrainableSAM(predictor.model)
    for n, p in model.sam.named_parameters():
        p.requires_grad_(n.startswith("mask_decoder."))
    unetr = U.UNETR(model.sam.image_encoder, U._default_widths(256, 3, True))       # transposed-convolution up-samplers
    for name, child in unetr.named_children():
        if name != "encoder":
            child.to("cuda")
    sam_params = [p for p in model.parameters() if p.requires_grad]
    dec_params = [p for n, p in unetr.named_parameters() if not n.startswith("encoder")]
    opt = torch.optim.AdamW(sam_params + dec_params, lr=1e-4)
    snaps = []
    opt.register_step_post_hook(lambda *_: snaps.append(([p.detach().clone() for p in sam_params], [p.detach().clone() for p in dec_params])))
    first = ([p.detach().clone() for p in sam_params], [p.detach().clone() for p in dec_params])
    trainer = JointSamTrainer(unetr=unetr, model=model, optimizer=opt, convert_inputs=ConvertToSamInputs(transform=model.transform),
                              n_sub_iteration=2, n_objects_per_batch=4, mask_prob=0.5)
    trainer.fit(ITERATIONS, [(x, y)])
    return trainer, snaps, first


def _moved(a, b):
    return sum(int(not torch.equal(p, q)) for p, q in zip(a, b))


@pytest.fixture(scope="module")
def runs(vit_b_sd):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from micro_sam_amd.training import PerObjectDistanceTransform
    image, x, y1 = _data()
    y4 = PerObjectDistanceTransform(instances=True, min_size=25)(y1[0, 0].cuda()).cpu()[None]      # the reference's four-channel layout
    with torch.backends.cudnn.flags(enabled=False):                    # (see the module docstring; restored when the module is done)
        yield image, x, y1, y4, _run(vit_b_sd, x, y1), _run(vit_b_sd, x, y4)


def test_each_pass_moves_its_own_parameters(runs):
    _, _, _, y4, (trainer, snaps, first), _ = runs
    assert y4.shape == (1, 4, 256, 256) and y4[0, 0].max() >= 5
    assert len(snaps) == 2 * ITERATIONS                                  # two optimizer steps per iteration
    sam0, dec0 = first
    sam1, dec1 = snaps[0]
    sam2, dec2 = snaps[1]
    assert _moved(sam0, sam1) == len(sam0) and _moved(dec0, dec1) == 0   # pass 1: the mask decoder moves, the UNETR decoder does not
    assert _moved(dec1, dec2) == len(dec0) and _moved(sam1, sam2) == 0   # pass 2: the other way round
    for rec in trainer.history:
        print(rec)
        assert set(rec) >= {"iteration", "loss", "mask_loss", "iou_regression_loss", "model_iou", "instance_loss"}
        assert all(np.isfinite(rec[k]) for k in ("loss", "instance_loss")) and 0 < rec["instance_loss"] <= 3
    assert [r["iteration"] for r in trainer.history] == list(range(ITERATIONS))


def test_one_channel_and_four_channel_labels_give_the_same_records(runs):
    _, _, _, _, (t1, _, _), (t4, _, _) = runs
    for a, b in zip(t1.history, t4.history):
        print("1 channel :", a)
        print("4 channels:", b)
    assert t1.history == t4.history
    same = sum(int(torch.equal(p, q)) for p, q in zip(t1.unetr.state_dict().values(), t4.unetr.state_dict().values()))
    print("UNETR tensors equal after the two runs:", same, "of", len(t1.unetr.state_dict()))


def test_checkpoint_loads_through_get_predictor_and_decoder(runs, tmp_path):
    from micro_sam_amd import instance_segmentation as IS
    from micro_sam_amd import util
    image, x, y1, _, (trainer, _, _), _ = runs
    path = str(tmp_path / "joint.pt")
    trainer.save_checkpoint(path)
    state = torch.load(path, map_location="cpu", weights_only=True)
    assert state["iteration"] == ITERATIONS and not any(k.startswith("encoder") for k in state["decoder_state"])
    assert any(k.startswith("sam.image_encoder.") for k in state["model_state"])
    predictor, decoder = IS.get_predictor_and_decoder("vit_b", path, device="cuda")
    emb = util.precompute_image_embeddings(predictor, image, verbose=False)
    feats = torch.as_tensor(emb["features"]).float().cuda()
    got = decoder(feats, emb["input_size"], emb["original_size"])
    unetr = trainer.unetr.eval()
    with torch.no_grad():
        want = unetr.postprocess_masks(unetr.decode(feats), emb["input_size"], emb["original_size"])
    d = (got - want).abs()
    print("decoder of the checkpoint vs the trainer's UNETR: max", float(d.max()), "mean", float(d.mean()))
    assert got.shape == want.shape == (1, 3, 256, 256)
    assert np.allclose(got.cpu().numpy(), want.cpu().numpy(), atol=1e-4)
    # and back into a trainer: a parameter spoilt after saving is restored, the iteration too
    name, p = next((n, p) for n, p in trainer.unetr.named_parameters() if n.startswith("out_conv"))
    kept = p.detach().clone()
    with torch.no_grad():
        p.zero_()
    trainer._iteration = 0
    trainer.load_checkpoint(path)
    assert torch.equal(p, kept) and trainer._iteration == ITERATIONS
    metric = trainer.validate([(x, y1)])
    print("validation metric:", metric)
    assert np.isfinite(metric) and 0 < metric < 3
