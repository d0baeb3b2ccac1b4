"""How many launches a runner entry makes: the nodes of a graph captured around one call of the EAGER entry, the way the library's own
*_graph_create forms capture it (relaxed mode, on a stream of its own; the slices' internal streams fork from it and join back into
it).  The graph is counted and destroyed, never launched.  The HIP runtime is reached through the library's own handle
(tests/hip_runtime.py)."""
import ctypes

import torch

import hip_runtime


def captured_nodes(eng, suffix, args):
    """nodes of one call of eng.PREFIX + suffix with the C arguments `args` (an `_args` kind of the engine: every buffer exists and
    the workspace is initialised before the capture begins)"""
    lib, P = eng.h.lib, ctypes.c_void_p
    rt = hip_runtime.bind(lib)
    stream = torch.cuda.Stream(eng.device)
    torch.cuda.synchronize(eng.device)
    eng.h.set_stream(stream.cuda_stream)
    graph = P()
    assert rt.hipStreamBeginCapture(P(stream.cuda_stream), hip_runtime.RELAXED) == 0
    st = getattr(lib, eng.PREFIX + suffix)(*args)
    ended = rt.hipStreamEndCapture(P(stream.cuda_stream), ctypes.byref(graph))
    try:
        assert st == 0, lib.ivit_last_error(eng.h.h).decode()
        assert ended == 0 and graph.value
        n = rt.node_count(graph)
    finally:
        if graph.value:
            rt.hipGraphDestroy(graph)
        eng._use_current_stream()
    return n
