"""The few HIP runtime calls the tests make themselves (stream capture and graph replay), with their ctypes prototypes stated once.
The runtime is reached through the library's own handle (a ctypes.CDLL of libivit_hip.so), which resolves the runtime's symbols as the
library's dependencies: the tests then drive the very runtime the library launches into, and load no second copy of it."""
import ctypes

_P = ctypes.c_void_p
RELAXED = 2         # hipStreamCaptureModeRelaxed: the mode the library's own *_graph_create forms capture in

_PROTOTYPES = {
    "hipStreamBeginCapture": [_P, ctypes.c_int],                      # stream, mode
    "hipStreamEndCapture": [_P, _P],                                  # stream, hipGraph_t *
    "hipGraphGetNodes": [_P, _P, _P],                                 # graph, hipGraphNode_t * (or NULL), size_t *count
    "hipGraphDestroy": [_P],
    "hipGraphInstantiate": [_P, _P, _P, _P, ctypes.c_size_t],         # hipGraphExec_t *, graph, error node *, log buffer, its size
    "hipGraphLaunch": [_P, _P],                                       # exec, stream
    "hipGraphExecDestroy": [_P],
}


class Runtime:
    """rt.hipStreamBeginCapture(...) and the rest of _PROTOTYPES, each returning a hipError_t (0 = hipSuccess)"""
    def __init__(self, lib):
        for name, argtypes in _PROTOTYPES.items():
            fn = getattr(lib, name)
            fn.argtypes, fn.restype = argtypes, ctypes.c_int
            setattr(self, name, fn)

    def node_count(self, graph):
        n = ctypes.c_size_t()
        assert self.hipGraphGetNodes(graph, None, ctypes.byref(n)) == 0
        return int(n.value)


def bind(lib):
    return Runtime(lib)
