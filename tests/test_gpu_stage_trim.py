"""StageTrim as one call (Engine.stage_trim; 10X/runstages/RunStages.cc:56-156).  Bar: the result equals the composition of the parts
that are each pinned to the reference -- MowLawn (tests/mowref.py on tests/golden/mow/), DeleteEdges + Cleanup (tests/editref.py on
tests/golden/edit/), the hanging-end rule (editref.hanging_ends) and DeleteEdges + Cleanup again -- in a.hbv, a.inv, the paths and the
a.pathsX bytes, through the existing writers; its first edit gets exactly mow_lawn's selection."""
import numpy as np
import pytest

import a48xref
import editref
import mowref
from mowdev import Input

pytestmark = pytest.mark.gpu
CASES = ("hand_k48", "hand_k60", "adversarial", "synth_4k_dups")


@pytest.fixture(scope="module")
def engine(snk):
    import torch
    from supernova_amd.engine import Engine
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    e = Engine(0)
    yield e
    e.close()


@pytest.mark.parametrize("name", CASES)
def test_equals_the_composition_of_its_parts(engine, name, tmp_path):
    c = mowref.load(name)
    dels, scored, _ = mowref.restated(name)
    assert len(dels) > 0
    first = editref.delete_edges(c.a_hbv, c.inv, *c.paths, dels)
    support, hang = editref.hanging_ends(first.a_hbv, first.inv, first.n_edges, first.edges)
    second = editref.delete_edges(first.a_hbv, first.inv, first.offset, first.n_edges, first.edges, hang)
    inp = Input(c)
    before = [t.clone() for t in inp.tensors()]
    with inp.handle() as h:
        out = engine.stage_trim(inp.graph(h), *inp.reads(), inp.bc, inp.paths)
        only_mow, _, _ = engine.mow_lawn(inp.graph(h), *inp.reads(), inp.paths, out.dup)
    assert np.array_equal(out.dup, c.dup), "MarkDups inside the stage"
    assert np.array_equal(out.mow_dels, dels) and np.array_equal(out.mow_dels, only_mow) and np.array_equal(out.scored, scored), "the first selection"
    assert out.stats["first"]["n_deleted"] == len(dels) and out.stats["mow_dels"] == len(dels)
    assert np.array_equal(out.support, support) and np.array_equal(out.dels, hang) and out.stats["hang_dels"] == len(hang), "the second selection"
    out.write(tmp_path / "a.hbv", tmp_path / "a.inv")
    assert (tmp_path / "a.hbv").read_bytes() == second.a_hbv, "a.hbv"
    assert (tmp_path / "a.inv").read_bytes() == second.a_inv and np.array_equal(out.inv, second.inv), "a.inv"
    ne = out.n_edges.cpu().numpy().view(np.uint32)
    assert np.array_equal(out.offset.cpu().numpy(), second.offset) and np.array_equal(ne, second.n_edges) and np.array_equal(out.edges.cpu().numpy(), second.edges), "paths"
    index, data, _ = engine.zip_paths(out.h, *out.paths)
    g2 = a48xref.parse_hbv(second.a_hbv)
    w_index, w_data, _ = a48xref.zip_paths(second.offset, second.n_edges, second.edges, g2)
    assert a48xref.pathsx_bytes(index, data, len(ne)) == a48xref.pathsx_bytes(w_index, w_data, len(ne)), "a.pathsX bytes"
    assert all(bool((a == b).all()) for a, b in zip(before, inp.tensors())), "an input array changed"
    assert out.stats["mow"]["n_deleted_candidates"] * 2 >= len(dels) and out.stats["dups"]["n_dup_pairs"] == int(c.dup.sum())
