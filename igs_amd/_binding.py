"""What the binders of igs_amd.motion and igs_amd.tokens share: the autocast test that picks a compute dtype and the key under which
weights packed from a module's parameters are kept."""
import torch


def autocast_half(fn, x):
    """True when CUDA autocast to float16 is on for x's device type; bfloat16 autocast is refused."""
    if not (x.is_cuda and torch.is_autocast_enabled()):
        return False
    dt = torch.get_autocast_dtype("cuda") if hasattr(torch, "get_autocast_dtype") else torch.get_autocast_gpu_dtype()
    if dt != torch.float16:
        raise NotImplementedError(f"{fn}: autocast to {dt} is not supported (float16 only)")
    return True


def param_key(params):
    """Changes whenever a pack made from `params` is stale: a parameter's _version, data_ptr, dtype or device."""
    return tuple(None if p is None else (p._version, p.data_ptr(), p.dtype, p.device) for p in params)
