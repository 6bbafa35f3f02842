"""What a call through the C ABI takes from torch: a tensor's address, the current stream, the error for host tensors, and the
read-back of the loops that run on the device."""
import ctypes as C

import torch


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def read_loops(states, histories):
    """The one read-back of device-resident loops (csrc/device_loop.h) from lists of state [k,STATE] and history [k,max_iterations,16]
    tensors: (state_h [n,STATE], history_h [n,max_iterations,16], status [n] int, done [n] int: the records written), numpy."""
    state, history = torch.cat(states), torch.cat(histories)
    both = torch.cat([state.reshape(-1), history.reshape(-1)]).cpu().numpy()
    state_h, history_h = both[:state.numel()].reshape(state.shape), both[state.numel():].reshape(history.shape)
    return state_h, history_h, state_h[:, 12].astype(int), state_h[:, 13].astype(int)


def no_cpu(what, why):
    return RuntimeError(f"{what} needs device tensors: {why}, there is no CPU path")
