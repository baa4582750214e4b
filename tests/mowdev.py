"""What the GPU tests of MowLawn and StageTrim share: a case of tests/mowref.py / tests/mowgen.py on the device."""
import numpy as np

import pathgen


def dev(a, dtype):
    import torch
    return torch.from_numpy(np.ascontiguousarray(np.array(a, dtype=dtype))).to(torch.device("cuda", 0))


class Input:
    """the unitigs in the order the graph names them, the reads, the paths; graph(h) is the tuple the engine takes"""

    def __init__(self, c):
        from supernova_amd import graphio
        self.c = c
        self.u = graphio.unitigs_to_arrays(c.unitigs)
        self.d_off, self.d_bases = dev(self.u[0].astype(np.int64), np.int64), dev(self.u[1], np.uint8)
        self.L = c.codes.shape[1]
        self.rows, self.quals, self.lens, self.bc = pathgen.to_device(c.codes, c.quals, c.lens, np.asarray(c.bc, np.int32))
        self.inv = np.asarray(c.inv, np.int32).copy()
        off, ne, edges = c.paths
        self.paths = (dev(off, np.int32), dev(np.asarray(ne, np.uint32).view(np.int32), np.int32), dev(edges if len(edges) else np.zeros(1, np.int32), np.int32)[:len(edges)])

    def handle(self):
        from supernova_amd import graphio
        return graphio.hbv_handle(self.c.K, *self.u)

    def graph(self, h):
        return (self.c.K, h, self.d_off, self.d_bases, self.inv)

    def reads(self):
        return (self.rows, self.L, self.quals, self.lens)

    def tensors(self):
        return (self.d_off, self.d_bases, self.rows, self.quals, self.lens, self.bc, *self.paths)
