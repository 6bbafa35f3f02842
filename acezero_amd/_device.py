"""What a call through the C ABI takes from torch: a tensor's address, the current stream, and the error for host tensors."""
import ctypes as C

import torch


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def no_cpu(what, why):
    return RuntimeError(f"{what} needs device tensors: {why}, there is no CPU path")
