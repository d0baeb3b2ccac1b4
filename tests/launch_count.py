"""How many launches a runner entry makes: the nodes of a graph captured around one call of the EAGER entry, the way the library's own
*_graph_create forms capture it (relaxed mode, on a stream of its own; the slices' internal streams fork from it and join back into
it).  The graph is counted and destroyed, never launched.  The HIP runtime is reached through the library's own handle, which
resolves the runtime's symbols as the library's dependencies."""
import ctypes

import torch

_RELAXED = 2        # hipStreamCaptureModeRelaxed


def captured_nodes(eng, suffix, args):
    """nodes of one call of eng.PREFIX + suffix with the C arguments `args` (an `_args` kind of the engine: every buffer exists and
    the workspace is initialised before the capture begins)"""
    lib, P = eng.h.lib, ctypes.c_void_p
    begin, end, nodes, destroy = lib.hipStreamBeginCapture, lib.hipStreamEndCapture, lib.hipGraphGetNodes, lib.hipGraphDestroy
    begin.argtypes, end.argtypes, nodes.argtypes, destroy.argtypes = [P, ctypes.c_int], [P, P], [P, P, P], [P]
    for f in (begin, end, nodes, destroy):
        f.restype = ctypes.c_int
    stream = torch.cuda.Stream(eng.device)
    torch.cuda.synchronize(eng.device)
    eng.h.set_stream(stream.cuda_stream)
    graph, n = P(), ctypes.c_size_t()
    assert begin(P(stream.cuda_stream), _RELAXED) == 0
    st = getattr(lib, eng.PREFIX + suffix)(*args)
    ended = end(P(stream.cuda_stream), ctypes.byref(graph))
    try:
        assert st == 0, lib.ivit_last_error(eng.h.h).decode()
        assert ended == 0 and graph.value
        assert nodes(graph, None, ctypes.byref(n)) == 0
    finally:
        if graph.value:
            destroy(graph)
        eng._use_current_stream()
    return int(n.value)
