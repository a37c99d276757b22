"""The one cache of packed conv weights (ops/conv3x3.packed, repack), on the CPU
through the torch-op packers. The GPU side (one batched repack launch, same
addresses) is in test_trunk_routes.py, the values in test_trunk_composed.py."""
import torch


def test_pack_cache_on_the_cpu():
    """What captured graphs and the learners rely on, through the torch-op
    packers: a buffer keeps its address, the version check alone picks up an
    in-place update, repack() refreshes every kind that exists (and only
    those) even when the version did not move, a deepcopy has its own."""
    import copy

    from moolib_amd.ops import conv3x3 as c3

    torch.manual_seed(0)
    conv = torch.nn.Conv2d(4, 16, 3, padding=1)
    bufs = {kind: c3.packed(conv, kind) for kind in ("fwd", "c8")}
    ptrs = {kind: b.data_ptr() for kind, b in bufs.items()}
    assert set(conv._c3_packs) == {"fwd", "c8"}

    def fresh(m):
        return {kind: c3.PACKERS[kind](m.weight.detach()) for kind in m._c3_packs}

    def current(m):
        return all(torch.equal(c3.packed(m, kind), want) and c3.packed(m, kind).data_ptr() == ptrs[kind]
                   for kind, want in fresh(m).items())

    assert current(conv)
    with torch.no_grad():
        conv.weight.mul_(2)                      # bumps the version
    assert current(conv)
    twin = copy.deepcopy(conv)
    assert all(twin._c3_packs[k][1].data_ptr() != ptrs[k] for k in ptrs)
    conv.weight.data.add_(1)                     # does not bump it
    assert not torch.equal(c3.packed(conv), fresh(conv)["fwd"])
    c3.repack(torch.nn.Sequential(conv))
    assert current(conv) and set(conv._c3_packs) == {"fwd", "c8"}
    assert torch.equal(twin._c3_packs["fwd"][1], fresh(twin)["fwd"])   # untouched by conv's updates
