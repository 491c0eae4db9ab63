"""The two collectives of the multi-rank paths (sharded.py, data_parallel.py), chosen by the process group's backend.

`nccl` (RCCL): the torch.distributed call itself -- same arguments, same async_op, ordered against torch's current
stream -- nothing is added in front of or behind it.

Any other backend (`gloo`: ranks as processes without RCCL, e.g. several ranks on ONE GPU, where RCCL refuses a second
rank per device): CPU tensors go to torch.distributed unchanged; a device tensor is staged through the host for the
collective only -- synchronise torch's current stream (the stream the library was handed, so its raw-pointer writes are
done), copy to the host, run the CPU collective, copy back on the current stream -- and the returned work object's
wait() has nothing left to wait for.  The overlap of a gather with the next block's sweep (ShardedIndex.score_topk) is
lost on that path; it is a correctness path, not a fast one.

The choice is made by backend name, never by probing what a torch build accepts: per torch's documentation gloo
carries device tensors for broadcast and all_reduce only, whatever ProcessGroupGloo of one build happens to take.
(Measured once on an MI355X with the ROCm build of torch the tests run on, staging switched off by hand: gloo took the
device tensors of all three product all_gather_into_tensor sites -- ShardedIndex.score_topk,
DataParallelTrainer._rows_sum_max, ._exchange_sparse -- and of the arena all_reduce, with right results; it refused only
the STACKED form all_gather_topk uses, [world, Q, k] from [Q, k], with "invalid tensor size", which is why the staged
gather runs on flat host tensors.  The staging stays: that acceptance is undocumented.)
"""


class _Done(object):
    """Work handle of a collective that has already completed."""

    def wait(self, timeout=None):
        return True


def _host_staged(tensor, group):
    import torch.distributed as dist
    return tensor.is_cuda and dist.get_backend(group) != "nccl"


def all_gather_into(out, inp, group=None, async_op=False):
    """dist.all_gather_into_tensor(out, inp): out is the ranks' `inp` concatenated along dim 0."""
    import torch
    import torch.distributed as dist
    if not _host_staged(out, group):
        return dist.all_gather_into_tensor(out, inp, group=group, async_op=async_op)
    torch.cuda.current_stream(inp.device).synchronize()
    # flat on the host: gloo takes the concatenation form only, RCCL also the stacked one ([world, ...] from [...])
    host_out = torch.empty(out.numel(), dtype=out.dtype)
    dist.all_gather_into_tensor(host_out, inp.cpu().reshape(-1), group=group)
    out.copy_(host_out.view(out.shape))
    return _Done() if async_op else None


def all_reduce_(tensor, group=None, async_op=False):
    """dist.all_reduce(tensor) (sum), in place."""
    import torch
    import torch.distributed as dist
    if not _host_staged(tensor, group):
        return dist.all_reduce(tensor, group=group, async_op=async_op)
    torch.cuda.current_stream(tensor.device).synchronize()
    host = tensor.cpu().contiguous()
    dist.all_reduce(host, group=group)
    tensor.copy_(host)
    return _Done() if async_op else None
