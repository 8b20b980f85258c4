"""The host restatement of the GINE stage's front record (signnet_basisnet_amd/gnn_front.py) against the pieces of the oracle it
restates: DiscreteEncoder rows (oracle.pyg_signnet.discrete_encoder) and PyG's in-edge order (gine_aggregate sums a node's
messages in edge-id order).  No GPU."""
import numpy as np
import pytest
import torch

import gnn_front_cases as cases
from oracle import pyg_signnet as O
from signnet_basisnet_amd import gnn_front as GF

D, L = 128, 2


@pytest.fixture(scope="module")
def sd():
    g = torch.Generator().manual_seed(11)
    sd = {"gnn.input_encoder.embeddings.0.weight": torch.randn(500, D, generator=g)}
    for l in range(L):
        sd[f"gnn.edge_encoders.{l}.embeddings.0.weight"] = torch.randn(500, D, generator=g)
    return sd


def _records(sd, data):
    ntab = sd["gnn.input_encoder.embeddings.0.weight"]
    etabs = [sd[f"gnn.edge_encoders.{l}.embeddings.0.weight"] for l in range(L)]
    return [GF.host_record(g, data.batch, data.edge_index, data.x, data.edge_attr, ntab, etabs) for g in range(data.num_graphs)]


@pytest.mark.parametrize("name", ["batch_one", "batch_three"])
def test_host_record_restates_the_oracle(sd, name):
    data = getattr(cases, name)()
    recs = _records(sd, data)
    assert all(r["valid"] for r in recs)
    enc = O.discrete_encoder(sd, "gnn.input_encoder", data.x.squeeze(-1))
    h = torch.randn(data.num_nodes, D, generator=torch.Generator().manual_seed(5))
    for l in range(L):
        e = O.discrete_encoder(sd, f"gnn.edge_encoders.{l}", data.edge_attr)
        want = O.gine_aggregate(h, data.edge_index, e, 0.0) - h             # sum over in-edges of relu(h_j + e_ji)
        for r in recs:
            gs, n = r["gs"], r["n"]
            assert torch.equal(r["enc"], enc[gs:gs + n])
            # every CSR slot's table row is its edge's embedding; slots of a node: ascending edge ids (PyG's summation order)
            rows = torch.from_numpy(r["ee"])[l * r["ncls"] + torch.from_numpy(r["ecls"]).long()] if r["ne"] else torch.zeros(0, D)
            assert torch.equal(rows, e[r["eid"]])
            got = torch.zeros(n, D)
            for row in range(n):
                dg, sr, er, lo = (int(v) for v in r["info"][row])
                ids = r["eid"][lo:lo + dg].tolist()
                assert ids == sorted(ids) and all(int(data.edge_index[1, i]) == gs + row for i in ids)
                for k in range(dg):
                    src = int(r["esrc"][lo + k])
                    assert src == int(data.edge_index[0, ids[k]]) - gs
                    if k < 4:
                        assert ((sr & 0xffffffff) >> (8 * k)) & 255 == src and ((er & 0xffffffff) >> (8 * k)) & 255 == int(r["ecls"][lo + k])
                    got[row] += torch.relu(h[gs + src] + rows[lo + k])
                for k in range(dg, 4):
                    assert ((sr & 0xffffffff) >> (8 * k)) & 255 == 64 and ((er & 0xffffffff) >> (8 * k)) & 255 == 255
            assert torch.allclose(got, want[gs:gs + n], rtol=0, atol=1e-5 * float(want.abs().max() + 1))
            assert int(r["info"][n:, 0].max(initial=-1)) == -1 and r["info"][:n, 0].sum() == r["ne"]


def test_shapes_reach_every_branch(sd):
    recs = _records(sd, cases.batch_three())
    assert [(r["n"] + 15) // 16 for r in recs] == [1, 2, 4] and recs[2]["ne"] == 192
    assert {0, 4, 9} <= set(recs[0]["info"][:16, 0].tolist())
    assert all(r["ncls"] == 2 for r in recs)
    assert _records(sd, cases.batch_one())[0]["ne"] == 0


def test_graphs_a_record_cannot_describe(sd):
    assert [r["valid"] for r in _records(sd, cases.batch_oversize())] == [1, 0, 1]
    assert [r["valid"] for r in _records(sd, cases.batch_bad_atom())] == [0, 1]
    d = cases.batch_three()
    d.batch = d.batch.flip(0)                                    # unsorted batch vector: no graph has a record
    assert [r["valid"] for r in _records(sd, d)] == [0, 0, 0]
    d = cases.batch_three()
    d.edge_index[0, 0] = d.num_nodes - 1                         # an edge across graphs: its destination's graph has no record
    assert [r["valid"] for r in _records(sd, d)][0] == 0
