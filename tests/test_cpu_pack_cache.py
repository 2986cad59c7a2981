"""Host-side bookkeeping of the packed-weight caches (ops.PackCache, ops.parameters_written), checked without a GPU:
which Parameters a cache is keyed by after copy / pickle / load_state_dict(assign=True), when a cached pack counts as
current, and that the data-parallel broadcast reports its raw writes.  What the packs CONTAIN is checked on the GPU
(tests/test_gpu_pack_freshness.py)."""
import copy
import gc
import os
import pickle
import socket
import weakref

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp


def _cached_unet(monkeypatch):
    """A UNet on the CPU with the pack cache model._pack_cache attaches, minus the device work (refresh)."""
    import tiaozhanbei_unet_amd as P
    from tiaozhanbei_unet_amd import model as M, ops
    monkeypatch.setattr(ops.PackCache, "refresh", lambda self, force=False: None)
    monkeypatch.setattr(ops, "_active_packs", None)
    torch.manual_seed(0)
    m = P.UNet(3, 2, precision="bf16")
    cache = M._pack_cache(m)
    assert m.__dict__["_packs"] is cache and len(cache.items) == 2 * (18 + 4) == len(cache.slots)
    return m


@pytest.fixture
def cached_unet(monkeypatch):
    return _cached_unet(monkeypatch)


def _own_keys(model):
    return {id(p) for p in model.parameters()}


def _check_cache_is_own_or_absent(model):
    cache = model.__dict__.get("_packs")
    if cache is None:
        return
    own = _own_keys(model)
    assert all(key[0] in own for key in cache.slots), "the cache is keyed by another model's Parameters"
    assert all(id(item[0]) in own for item in cache.items)
    assert all((id(w), m) in cache.slots for (w, m, _, _, _) in cache.items)


def test_deepcopy_carries_no_foreign_pack_cache(cached_unet):
    m = cached_unet
    c = copy.deepcopy(m)
    _check_cache_is_own_or_absent(c)
    assert "_packs" in m.__dict__, "copying must leave the original's cache alone"
    _check_cache_is_own_or_absent(m)
    from tiaozhanbei_unet_amd import model as M
    cache = M._pack_cache(c)                          # the copy's next forward: a cache of its own
    assert cache is not m.__dict__["_packs"] and cache is c.__dict__["_packs"]
    _check_cache_is_own_or_absent(c)


def test_pickle_carries_no_pack_cache(cached_unet):
    m = cached_unet
    state = m.__reduce_ex__(2)[2]
    assert "_packs" not in state
    c = pickle.loads(pickle.dumps(m))
    assert "_packs" not in c.__dict__
    for (k, a), (_, b) in zip(m.state_dict().items(), c.state_dict().items()):
        assert torch.equal(a, b), k
    assert c.compute_dtype == torch.bfloat16


def test_averaged_model_copy_has_its_own_cache(cached_unet):
    avg = torch.optim.swa_utils.AveragedModel(cached_unet)
    _check_cache_is_own_or_absent(avg.module)


def test_cache_follows_replaced_parameters(cached_unet):
    from tiaozhanbei_unet_amd import model as M
    m = cached_unet
    old_cache = m.__dict__["_packs"]
    assert M._pack_cache(m) is old_cache              # nothing replaced: the cache stays
    old = weakref.ref(m.down2.maxpool_conv[1].double_conv[3].weight)
    old_t = weakref.ref(m.up3.up.weight)
    state = {k: v.detach().clone() * 1.5 for k, v in m.state_dict().items()}
    m.load_state_dict(state, assign=True)
    assert m.up3.up.weight is not old_t()
    cache = M._pack_cache(m)
    assert cache is not old_cache
    _check_cache_is_own_or_absent(m)
    del old_cache
    gc.collect()
    assert old() is None and old_t() is None, "the replaced Parameters are still held"
    assert M._pack_cache(m) is cache


def test_active_cache_does_not_outlive_its_model(monkeypatch):
    """ops keeps the cache of the model that ran last for the operators' lookups -- not alive: a deleted model's packs
    and weights go with it, and a lookup afterwards packs for itself."""
    from tiaozhanbei_unet_amd import ops
    m = _cached_unet(monkeypatch)
    w = weakref.ref(m.inc.double_conv[3].weight)
    cache = weakref.ref(m.__dict__["_packs"])
    del m
    gc.collect()
    assert cache() is None and w() is None
    calls = []
    monkeypatch.setattr(ops, "pack_weight", lambda *a, **k: calls.append(a) or "packed")
    t = torch.zeros(64, 64, 3, 3)
    assert ops.packed(t, ops.L.PACK_CONV_FWD, 64, 64, torch.bfloat16) == "packed" and len(calls) == 1


def test_cached_pack_is_current_until_a_version_moves_or_parameters_are_written(cached_unet):
    import tiaozhanbei_unet_amd as P
    from tiaozhanbei_unet_amd import ops
    assert P.parameters_written is ops.parameters_written and "parameters_written" in P.__all__
    cache = cached_unet.__dict__["_packs"]
    w = cached_unet.up4.conv.double_conv[3].weight
    slot = cache.slots[(id(w), ops.L.PACK_CONV_DGRAD)]
    view = object()
    slot[0], slot[3] = view, w._version               # what _build + refresh leave behind
    cache.wgen = ops._write_generation
    args = (w, ops.L.PACK_CONV_DGRAD, slot[1], slot[2], slot[4])
    assert cache.get(*args) is view
    assert cache.get(w, ops.L.PACK_CONV_DGRAD, slot[1] + 64, slot[2], slot[4]) is None
    g0 = ops._train_generation
    w.data.mul_(1.5)                                   # moves no version counter ...
    assert cache.get(*args) is view
    P.parameters_written()                             # ... hence the contract
    assert ops._train_generation == g0 + 1
    assert cache.get(*args) is None
    cache.wgen = ops._write_generation
    assert cache.get(*args) is view
    with torch.no_grad():
        w.mul_(1.5)
    assert cache.get(*args) is None


def test_cache_watches_the_models_buffers(cached_unet):
    """A write to any buffer of the model (what AveragedModel.update_parameters does to all of them) is a witness that
    the model was rewritten, for writers whose parameter updates move no version counter."""
    cache = cached_unet.__dict__["_packs"]
    buffers = list(cached_unet.buffers())
    assert len(cache.witnesses) == len(buffers) == 18 * 3 and all(a is b for a, b in zip(cache.witnesses, buffers))
    seen = [b._version for b in cache.witnesses]
    cached_unet.up2.conv.double_conv[4].num_batches_tracked.detach().copy_(torch.tensor(3))
    assert seen != [b._version for b in cache.witnesses]


# ------------------------------------------------------------------ the data-parallel broadcast reports its writes
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _net(seed):
    torch.manual_seed(seed)
    return torch.nn.Sequential(torch.nn.Conv2d(3, 8, 3), torch.nn.BatchNorm2d(8), torch.nn.Conv2d(8, 2, 1))


def _broadcast_worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from tiaozhanbei_unet_amd import ops
        from tiaozhanbei_unet_amd.ddp import DataParallel
        net = _net(100 + rank)
        with torch.no_grad():
            net[1].running_mean.fill_(float(rank + 1))
        before = [t.detach().clone() for t in list(net.parameters()) + list(net.buffers())]
        versions = [p._version for p in net.parameters()]
        gen = (ops._train_generation, ops._write_generation)
        DataParallel(net, bucket_bytes=1024)
        after = [t.detach().clone() for t in list(net.parameters()) + list(net.buffers())]
        out[rank] = (before, after, versions == [p._version for p in net.parameters()],
                     ops._train_generation - gen[0], ops._write_generation - gen[1])
    finally:
        dist.destroy_process_group()


def test_data_parallel_broadcast_reports_parameters_written():
    """Rank 1 receives rank 0's weights through ``param.data`` (no version counter moves): the construction of
    DataParallel must bump the generation that every packed copy is stamped with."""
    world, port = 2, _free_port()
    mgr = mp.get_context("spawn").Manager()
    out = mgr.dict()
    mp.spawn(_broadcast_worker, args=(world, port, out), nprocs=world, join=True)
    b0, a0, _, _, _ = out[0]
    b1, a1, versions_kept, dgen, dwgen = out[1]
    for x, y in zip(a1, b0):
        assert torch.equal(x, y), "rank 1 does not hold rank 0's values after the broadcast"
    assert any(not torch.equal(x, y) for x, y in zip(a1[:6], b1[:6])), "the broadcast changed no parameter of rank 1"
    assert not torch.equal(a1[6], b1[6]), "running_mean of rank 1 kept its own value"
    assert versions_kept, "(the reason for the call: the broadcast writes param.data)"
    assert dgen >= 1 and dwgen >= 1, "rank 1's packed copies still count as current"
