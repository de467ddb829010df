"""GPU suite (-m gpu): the forms of TrainEngine's camera-gradient steps (step_on_image / step_on_views / localize_on_image /
localize_on_views with pose_grad(s), cameras, intrinsics) through the public API alone -- what each refuses, with which exception
and message, and which kernels one step of each form launches, how often.  The launch counts are compared with the committed
tests/step_launches.json, recorded by this module:

    python tests/test_gpu_step_forms.py --record tests/step_launches.json

The step scene of tests/engine_scenes.py: its small nets, 8 + 8 samples, 256 rays, V = 3, the dense backward."""
import json
import sys

import pytest
import torch

import conftest  # noqa: F401 (first: run as a script, --record, this is what puts the package and the oracle on sys.path)
import engine_scenes as ES

pytestmark = pytest.mark.gpu

FIXTURE = ES.STEP_LAUNCHES
V = ES.V


# ---- a. refusals ------------------------------------------------------------------------------------------------------------------------
def _refusals(s):
    """(label, call, exception type, message substring): what the engine raises, first violation first."""
    dev = s.dev
    one, two = s.engine(world_size=1), s.engine(world_size=2)
    T, I = s.table(), s.intrinsics()
    img, vw, no_poses = s.image_args(), s.views_args(), s.views_args(poses=False)
    g34 = lambda: torch.empty(3, 4, device=dev)  # noqa: E731
    gv34 = lambda: torch.empty(V, 3, 4, device=dev)  # noqa: E731
    tensor_intr = torch.tensor([s.focal, s.focal, s.W * 0.5, s.H * 0.5], device=dev)
    rays, tgt = torch.zeros(64, 11, device=dev), torch.zeros(64, 3, device=dev)
    R, NI = RuntimeError, NotImplementedError
    not_34 = "pose_grad must be a contiguous float32 (3, 4) tensor"
    not_v34 = "pose_grads must be a contiguous float32 (%d, 3, 4) tensor" % V
    not_intr = "intrinsics must be a cameras.Intrinsics (got Tensor)"
    rows = [
        # one violation
        ("image: pose_grad shape", lambda: one.step_on_image(*img, pose_grad=torch.empty(4, 4, device=dev)), R, not_34),
        ("image: pose_grad dtype", lambda: one.step_on_image(*img, pose_grad=torch.empty(3, 4, device=dev, dtype=torch.float64)), R, not_34),
        ("image: pose_grad strides", lambda: one.step_on_image(*img, pose_grad=torch.empty(4, 3, device=dev).t()), R, not_34),
        ("localize image: pose_grad shape", lambda: one.localize_on_image(*img, pose_grad=torch.empty(3, 3, device=dev)), R, not_34),
        ("localize image: pose_grad strides", lambda: one.localize_on_image(*img, pose_grad=torch.empty(3, 8, device=dev)[:, ::2]), R, not_34),
        ("views: pose_grads V", lambda: one.step_on_views(*vw, pose_grads=torch.empty(V + 1, 3, 4, device=dev)), R, not_v34),
        ("localize views: pose_grads V", lambda: one.localize_on_views(*vw, pose_grads=torch.empty(V - 1, 3, 4, device=dev)), R, not_v34),
        ("views: cameras with poses", lambda: one.step_on_views(*vw, cameras=T), R, "pass poses=None"),
        ("localize views: cameras with poses", lambda: one.localize_on_views(*vw, cameras=T), R, "pass poses=None"),
        ("views: cameras with pose_grads", lambda: one.step_on_views(*no_poses, pose_grads=gv34(), cameras=T), R, "exclude each other"),
        ("localize views: cameras with pose_grads", lambda: one.localize_on_views(*no_poses, pose_grads=gv34(), cameras=T), R,
         "exclude each other"),
        ("image: tensor intrinsics", lambda: one.step_on_image(*img, intrinsics=tensor_intr), R, not_intr),
        ("views: tensor intrinsics", lambda: one.step_on_views(*vw, intrinsics=tensor_intr), R, not_intr),
        ("localize image: tensor intrinsics", lambda: one.localize_on_image(*img, intrinsics=tensor_intr), R, not_intr),
        ("localize views: tensor intrinsics", lambda: one.localize_on_views(*vw, intrinsics=tensor_intr), R, not_intr),
        ("localize image: nothing asked", lambda: one.localize_on_image(*img), R, "localize_on_image needs pose_grad=... or intrinsics=..."),
        ("localize views: nothing asked", lambda: one.localize_on_views(*vw), R,
         "localize_on_views needs pose_grads=..., cameras=... or intrinsics=..."),
        ("forward_backward: frozen without ray_grad", lambda: one.forward_backward(rays, tgt, frozen=True), R,
         "forward_backward(frozen=True) computes the ray gradient alone: pass ray_grad=..."),
        ("forward_backward: ray_grad shape", lambda: one.forward_backward(rays, tgt, ray_grad=torch.empty(64, 8, device=dev)), R,
         "ray_grad must be a contiguous float32 tensor of the rays' shape (64, 11)"),
        ("forward_backward: ray_grad strides", lambda: one.forward_backward(rays, tgt, ray_grad=torch.empty(11, 64, device=dev).t(),
                                                                            frozen=True), R, "ray_grad must be a contiguous float32 tensor"),
        ("two ranks: pose_grad", lambda: two.step_on_image(*img, pose_grad=g34()), NI, "pose_grad with world size 2"),
        ("two ranks: pose_grads", lambda: two.step_on_views(*vw, pose_grads=gv34()), NI, "pose_grads with world size 2"),
        ("two ranks: cameras", lambda: two.step_on_views(*no_poses, cameras=T), NI, "cameras with world size 2"),
        ("two ranks: intrinsics, image", lambda: two.step_on_image(*img, intrinsics=I), NI, "intrinsics with world size 2"),
        ("two ranks: intrinsics, views", lambda: two.step_on_views(*vw, intrinsics=I), NI, "intrinsics with world size 2"),
        ("two ranks: localize_on_image", lambda: two.localize_on_image(*img, pose_grad=g34()), NI, "localize_on_image with world size 2"),
        ("two ranks: localize_on_views", lambda: two.localize_on_views(*no_poses, cameras=T), NI, "localize_on_views with world size 2"),
        ("two ranks: ray_grad", lambda: two.forward_backward(rays, tgt, ray_grad=torch.empty_like(rays)), NI, "ray_grad with world size 2"),
        # two violations: the first one in the step's order speaks
        ("views: cameras with poses, tensor intrinsics", lambda: one.step_on_views(*vw, cameras=T, intrinsics=tensor_intr), R, not_intr),
        ("localize views: cameras with poses, tensor intrinsics", lambda: one.localize_on_views(*vw, cameras=T, intrinsics=tensor_intr), R,
         not_intr),
        ("two ranks, views: cameras with poses", lambda: two.step_on_views(*vw, cameras=T), R, "pass poses=None"),
        ("two ranks, localize views: cameras with poses", lambda: two.localize_on_views(*vw, cameras=T), NI,
         "localize_on_views with world size 2"),
        ("two ranks, views: intrinsics, cameras with poses", lambda: two.step_on_views(*vw, cameras=T, intrinsics=I), NI,
         "intrinsics with world size 2"),
        ("two ranks, views: tensor intrinsics", lambda: two.step_on_views(*vw, intrinsics=tensor_intr), R, not_intr),
        ("image: pose_grad shape, tensor intrinsics", lambda: one.step_on_image(*img, pose_grad=torch.empty(4, 4, device=dev),
                                                                                intrinsics=tensor_intr), R, not_34),
        ("two ranks, image: pose_grad shape", lambda: two.step_on_image(*img, pose_grad=torch.empty(4, 4, device=dev)), NI,
         "pose_grad with world size 2"),
        ("two ranks, localize image: nothing asked", lambda: two.localize_on_image(*img), NI, "localize_on_image with world size 2"),
        ("views: cameras with poses and pose_grads", lambda: one.step_on_views(*vw, pose_grads=gv34(), cameras=T), R, "pass poses=None"),
        ("views: pose_grads V, tensor intrinsics", lambda: one.step_on_views(*vw, pose_grads=torch.empty(V + 1, 3, 4, device=dev),
                                                                            intrinsics=tensor_intr), R, not_intr),
        ("two ranks, forward_backward: frozen without ray_grad", lambda: two.forward_backward(rays, tgt, frozen=True), R,
         "computes the ray gradient alone"),
    ]
    return rows, (one, two, T, I)


def test_step_forms_refuse_what_they_cannot_do():
    rows, (one, two, T, I) = _refusals(ES.Scene())
    wrong = []
    for label, call, exc, text in rows:
        try:
            call()
        except Exception as e:  # noqa: BLE001 (the type is what is compared)
            if type(e) is not exc or text not in str(e):
                wrong.append((label, type(e).__name__, str(e)))
        else:
            wrong.append((label, None, "no exception"))
    torch.cuda.synchronize()
    assert not wrong, wrong
    # a refused call has not stepped anything
    assert one.step_count == two.step_count == one.localize_count == two.localize_count == T.step_count == I.step_count == 0
    assert torch.all(T.xi == 0) and torch.all(I.q == 0)


# ---- b. launch counts -------------------------------------------------------------------------------------------------------------------
def _forms(s):
    """{form: (engine, cameras, intrinsics) -> one step of that form}."""
    dev = s.dev
    img, vw, no_poses = s.image_args(), s.views_args(), s.views_args(poses=False)
    g34 = lambda: torch.empty(3, 4, device=dev)  # noqa: E731
    gv34 = lambda: torch.empty(V, 3, 4, device=dev)  # noqa: E731
    return {
        "step_on_image": lambda e, T, I: e.step_on_image(*img),
        "step_on_image pose_grad": lambda e, T, I: e.step_on_image(*img, pose_grad=g34()),
        "step_on_image intrinsics": lambda e, T, I: e.step_on_image(*img, intrinsics=I),
        "step_on_image pose_grad intrinsics": lambda e, T, I: e.step_on_image(*img, pose_grad=g34(), intrinsics=I),
        "step_on_views": lambda e, T, I: e.step_on_views(*vw),
        "step_on_views pose_grads": lambda e, T, I: e.step_on_views(*vw, pose_grads=gv34()),
        "step_on_views cameras": lambda e, T, I: e.step_on_views(*no_poses, cameras=T),
        "step_on_views intrinsics": lambda e, T, I: e.step_on_views(*vw, intrinsics=I),
        "step_on_views cameras intrinsics": lambda e, T, I: e.step_on_views(*no_poses, cameras=T, intrinsics=I),
        "localize_on_image pose_grad": lambda e, T, I: e.localize_on_image(*img, pose_grad=g34()),
        "localize_on_image intrinsics": lambda e, T, I: e.localize_on_image(*img, intrinsics=I),
        "localize_on_views pose_grads": lambda e, T, I: e.localize_on_views(*vw, pose_grads=gv34()),
        "localize_on_views cameras": lambda e, T, I: e.localize_on_views(*no_poses, cameras=T),
        "localize_on_views cameras intrinsics": lambda e, T, I: e.localize_on_views(*no_poses, cameras=T, intrinsics=I),
    }


def _launches():
    """{form: {kernel name: launches}} of the second step of every form (the first one warms up), a fresh engine, table and
    Intrinsics for each."""
    s = ES.Scene()
    return ES.form_launches(s, _forms(s), lambda: (s.engine(world_size=1), s.table(), s.intrinsics()))


def test_every_step_form_launches_what_the_fixture_recorded():
    with open(FIXTURE) as f:
        want = json.load(f)
    got = _launches()
    assert sorted(got) == sorted(want) and len(got) == 14
    for form in want:
        assert got[form] and got[form] == want[form], (form, got[form], want[form])


if __name__ == "__main__":
    if len(sys.argv) != 3 or sys.argv[1] != "--record":
        sys.exit("usage: python tests/test_gpu_step_forms.py --record PATH")
    with open(sys.argv[2], "w") as f:
        json.dump(_launches(), f, indent=1, sort_keys=True)
        f.write("\n")
