"""wrw_fold_grouped: the ordered fold of the weight-gradient partial planes,
for up to four layers in one launch. Held bit for bit to
torch_ref.wrw_fold_ordered (itself tested on the CPU in
tests/test_wrw_fold_ref.py) on random planes, no wrw kernel involved, and a
grouped launch to the same jobs folded one at a time."""

import pytest
import torch

from distributed_rl_amd.ops import torch_ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
PLANES = [1, 15, 16, 17, 63, 64, 65, 128]


@pytest.fixture(scope="module")
def ext():
    from distributed_rl_amd.ops import hip_ext

    return hip_ext(required=True)


@pytest.fixture(scope="module")
def pad(ext):
    return ext.wrw_plane_pad()


def _job(pad, planes, n_elem, cout, b_planes, dtype, seed):
    """(part, mb, b_part, gw, gb): random planes (NaN in the pad columns,
    which nothing may read), NaN-prefilled outputs. cout None: no bias."""
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    part = torch.randn(planes, n_elem + pad, device=DEV, generator=g)
    part[:, n_elem:] = float("nan")
    gw = torch.full((n_elem,), float("nan"), dtype=dtype, device=DEV)
    if cout is None:
        e = torch.empty(0, device=DEV)
        return part, planes, e, gw, e
    b_part = torch.randn(b_planes, cout, device=DEV, generator=g)
    gb = torch.full((cout,), float("nan"), dtype=dtype, device=DEV)
    return part, planes, b_part, gw, gb


def _fold(ext, jobs):
    ext.wrw_fold_grouped([j[0] for j in jobs], [j[1] for j in jobs],
                         [j[2] for j in jobs], [j[3] for j in jobs],
                         [j[4] for j in jobs])
    torch.cuda.synchronize()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16],
                         ids=["f32", "bf16"])
@pytest.mark.parametrize("cout", [16, 32, 64])
@pytest.mark.parametrize("n_elem", [64, 8192])
@pytest.mark.parametrize("planes", PLANES)
def test_single_fold_matches_reference(ext, pad, planes, n_elem, cout, dtype):
    # the bias partials take the plane count too (256 in the wrw path)
    job = _job(pad, planes, n_elem, cout, planes, dtype,
               seed=planes * 7 + n_elem + cout)
    _fold(ext, [job])
    ref_w, ref_b = torch_ref.wrw_fold_ordered(job[0], n_elem, job[2], dtype)
    assert torch.equal(job[3].cpu(), ref_w)
    assert torch.equal(job[4].cpu(), ref_b)


def test_single_fold_256_bias_planes(ext, pad):
    job = _job(pad, 128, 2048, 32, 256, torch.bfloat16, seed=5)
    _fold(ext, [job])
    ref_w, ref_b = torch_ref.wrw_fold_ordered(job[0], 2048, job[2],
                                              torch.bfloat16)
    assert torch.equal(job[3].cpu(), ref_w)
    assert torch.equal(job[4].cpu(), ref_b)


# (planes, n_elem, cout or None, b_planes) per job: different sizes and
# plane counts, bias and no-bias jobs mixed, a no-bias job first and last
GROUPS = [
    [(17, 64, 16, 256), (128, 8192, None, 0)],
    [(65, 8192, None, 0), (1, 64, 64, 3), (63, 2048, 32, 256)],
    [(16, 2048, 64, 256), (128, 8192, 32, 256), (15, 64, None, 0),
     (64, 4096, 16, 17)],
    [(1, 64, None, 0), (2, 64, None, 0), (3, 64, None, 0), (4, 64, None, 0)],
]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16],
                         ids=["f32", "bf16"])
@pytest.mark.parametrize("group", GROUPS, ids=lambda g: f"{len(g)}jobs")
def test_grouped_fold_equals_single_folds(ext, pad, group, dtype):
    mk = lambda: [_job(pad, p, n, c, bp, dtype, seed=31 * i + p)
                  for i, (p, n, c, bp) in enumerate(group)]
    grouped, single = mk(), mk()
    _fold(ext, grouped)
    for j in single:
        _fold(ext, [j])
    for a, b in zip(grouped, single):
        assert torch.equal(a[0][:, :a[3].numel()], b[0][:, :b[3].numel()])
        assert not torch.isnan(a[3].float()).any()
        assert torch.equal(a[3], b[3])
        assert torch.equal(a[4], b[4])
        if a[4].numel():
            assert not torch.isnan(a[4].float()).any()


def test_grouped_fold_rejects_before_launch(ext, pad):
    def ok():
        return [_job(pad, 4, 64, 16, 8, torch.float32, seed=i)
                for i in range(2)]

    def untouched(jobs):
        torch.cuda.synchronize()
        return all(torch.isnan(j[3]).all() and torch.isnan(j[4]).all()
                   for j in jobs)

    jobs = ok() + ok() + ok()[:1]  # a fifth job
    with pytest.raises(RuntimeError):
        _fold(ext, jobs)
    assert untouched(jobs)
    jobs = ok()  # dtype mismatch between the jobs
    jobs[1] = _job(pad, 4, 64, 16, 8, torch.bfloat16, seed=9)
    with pytest.raises(RuntimeError):
        _fold(ext, jobs)
    assert untouched(jobs)
    jobs = ok()  # gb of another dtype than gw
    jobs[1] = jobs[1][:4] + (jobs[1][4].to(torch.bfloat16),)
    with pytest.raises(RuntimeError):
        _fold(ext, jobs)
    assert untouched(jobs)
    jobs = ok()  # short b_part: a row of 8 where cout is 16
    jobs[1] = jobs[1][:2] + (jobs[1][2][:, :8].contiguous(),) + jobs[1][3:]
    with pytest.raises(RuntimeError):
        _fold(ext, jobs)
    assert untouched(jobs)
    jobs = ok()  # b_part without gb
    jobs[0] = jobs[0][:4] + (torch.empty(0, device=DEV),)
    with pytest.raises(RuntimeError):
        _fold(ext, jobs)
    assert untouched(jobs[1:])
    jobs = ok()  # fewer planes than mb says
    jobs[0] = (jobs[0][0][:3].contiguous(),) + jobs[0][1:]
    with pytest.raises(RuntimeError):
        _fold(ext, jobs)
    assert untouched(jobs)
    jobs = ok()  # planes without the pad columns
    jobs[0] = (jobs[0][0][:, :64].contiguous(),) + jobs[0][1:]
    with pytest.raises(RuntimeError):
        _fold(ext, jobs)
    assert untouched(jobs)
    jobs = ok()  # n_elem that is no multiple of 64
    jobs[1] = jobs[1][:3] + (jobs[1][3][:32],) + jobs[1][4:]
    with pytest.raises(RuntimeError):
        _fold(ext, jobs)
    assert untouched(jobs)
    jobs = ok()  # planes on the host
    jobs[0] = (jobs[0][0].cpu(),) + jobs[0][1:]
    with pytest.raises(RuntimeError):
        _fold(ext, jobs)
    assert untouched(jobs)
