"""Raw-HIP stream capture for the tests that replay a scan plan from a graph (a helper module, not a test).

A CaptureStream is a non-blocking HIP stream to hand to impop_amd.Context(0, stream=cs.handle); capture(fn) records what fn
launches on it into a graph, instantiates it and returns a Graph, which knows how many nodes the capture took and replays on the
same stream.  Nothing here goes through torch: the calls are the runtime's own, on the one copy of it in the process."""
import ctypes as C

HIP_STREAM_NON_BLOCKING = 1
HIP_STREAM_CAPTURE_MODE_GLOBAL = 0


def hip_runtime():
    """the HIP runtime the library is bound to (the one copy in this process)"""
    from impop_amd import _lib
    _lib.load()  # loads the library, and with it the runtime
    with open("/proc/self/maps") as f:
        paths = {line.split()[-1] for line in f if "libamdhip64.so" in line}
    assert len(paths) == 1, paths
    return C.CDLL(paths.pop())


class Graph:
    def __init__(self, hip, stream, graph, gexec):
        self.hip, self.stream, self.graph, self.gexec = hip, stream, graph, gexec
        n = C.c_size_t(0)
        assert hip.hipGraphGetNodes(graph, None, C.byref(n)) == 0
        self.n_nodes = int(n.value)

    def replay(self):
        assert self.hip.hipGraphLaunch(self.gexec, self.stream) == 0

    def destroy(self):
        if self.gexec is not None:
            assert self.hip.hipGraphExecDestroy(self.gexec) == 0 and self.hip.hipGraphDestroy(self.graph) == 0
            self.gexec = self.graph = None


class CaptureStream:
    def __init__(self):
        self.hip = hip_runtime()
        self.stream = C.c_void_p()
        assert self.hip.hipStreamCreateWithFlags(C.byref(self.stream), HIP_STREAM_NON_BLOCKING) == 0

    @property
    def handle(self):
        return self.stream.value

    def synchronize(self):
        assert self.hip.hipStreamSynchronize(self.stream) == 0

    def capture(self, fn) -> Graph:
        """fn(): launches on the stream, and nothing else (no allocation, no synchronisation: the capture is global)"""
        graph, gexec = C.c_void_p(), C.c_void_p()
        self.synchronize()
        assert self.hip.hipStreamBeginCapture(self.stream, HIP_STREAM_CAPTURE_MODE_GLOBAL) == 0
        try:
            fn()
        finally:
            rc = self.hip.hipStreamEndCapture(self.stream, C.byref(graph))
        assert rc == 0, rc
        assert self.hip.hipGraphInstantiate(C.byref(gexec), graph, None, None, C.c_size_t(0)) == 0
        return Graph(self.hip, self.stream, graph, gexec)

    def destroy(self):
        if self.stream is not None:
            assert self.hip.hipStreamDestroy(self.stream) == 0
            self.stream = None
