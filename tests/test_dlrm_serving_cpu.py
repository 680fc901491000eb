"""dlrm_tiny through the serving core on the CPU, over real gRPC as
tests/test_server_e2e.py serves half_plus_two: Predict with two inputs; Classify
and Regress over serialized tf.Examples (one ParseExample with a float [13] and
an int64 [T] key) agree with Predict; a missing feature and a feature of the
wrong length give ParseExample's errors."""
import asyncio
import os

import numpy as np
import pytest

from rust_tensorflow_serving2_amd.client import TensorflowServing, TFServingError, unpack_signature_defs
from rust_tensorflow_serving2_amd.schema import serving
from rust_tensorflow_serving2_amd.server.server import ModelServer, ServerOptions

import grpc

T_SPARSE = 9          # dlrm_tiny: hotness 1 + 3 + 2 + 1 + 2


@pytest.fixture(scope="module")
def server(models_dir):
    from rust_tensorflow_serving2_amd.models import dlrm
    base = os.path.join(str(models_dir), "dlrm_served")
    dlrm.export(os.path.join(base, "1"), "dlrm_tiny", seed=5)
    cfg = serving.ModelServerConfig()
    cfg.model_config_list.config.add(name="dlrm", base_path=base, model_platform="tensorflow")
    srv = ModelServer(ServerOptions(port=0, model_config=cfg, file_system_poll_wait_seconds=0.2)).start()
    yield srv
    srv.stop()


def run(coro):
    return asyncio.run(coro)


async def client(port, sig=None):
    b = TensorflowServing.new().hostname("127.0.0.1").port(port)
    if sig:
        b = b.signature_name(sig)
    return await b.build()


def inputs(batch=4):
    from rust_tensorflow_serving2_amd.models import dlrm
    return dlrm.random_inputs("dlrm_tiny", batch, seed=2, ends=True)


def test_signatures(server):
    async def go():
        c = await client(server.port)
        sigs = unpack_signature_defs(await c.model_metadata("dlrm"))
        assert set(sigs) == {"serving_default", "classify", "regress"}
        assert set(sigs["serving_default"].inputs) == {"dense", "sparse"}
        assert [d.size for d in sigs["serving_default"].inputs["sparse"].tensor_shape.dim] == [-1, T_SPARSE]
        assert sigs["classify"].method_name == "tensorflow/serving/classify"
        assert sigs["regress"].method_name == "tensorflow/serving/regress"
    run(go())


def test_predict_with_two_inputs(server):
    dense, sparse = inputs()

    async def go():
        c = await client(server.port)
        out = await c.predict_tensors("dlrm", {"dense": dense, "sparse": sparse})
        assert set(out) == {"logits", "probabilities"}
        lg, pr = out["logits"].reshape(-1), out["probabilities"].reshape(-1)
        assert lg.shape == (4,) and np.ptp(lg) > 1e-3
        np.testing.assert_allclose(pr, 1 / (1 + np.exp(-lg.astype(np.float64))), atol=1e-6)
        # each row alone gives the same logit (nothing crosses the batch)
        one = await c.predict_tensors("dlrm", {"dense": dense[2:3], "sparse": sparse[2:3]})
        np.testing.assert_allclose(one["logits"].reshape(-1), lg[2:3], atol=1e-6)
    run(go())


def test_classify_and_regress_agree_with_predict(server):
    dense, sparse = inputs()

    async def go():
        p = await client(server.port)
        out = await p.predict_tensors("dlrm", {"dense": dense, "sparse": sparse})
        c = await client(server.port, "classify")
        r = await client(server.port, "regress")
        for i in range(len(dense)):
            example = {"dense": [float(v) for v in dense[i]], "sparse": [int(v) for v in sparse[i]]}
            res = await c.classify("dlrm", example)
            assert res.classifications[0].classes[0].score == pytest.approx(float(out["probabilities"][i, 0]), abs=1e-6)
            res = await r.regress("dlrm", example)
            assert res.regressions[0].value == pytest.approx(float(out["logits"][i, 0]), abs=1e-6)
    run(go())


@pytest.mark.parametrize("example,message", [
    ({"dense": [0.5] * 13}, "Feature: sparse (data type: int64) is required but could not be found"),
    ({"sparse": [0] * T_SPARSE}, "Feature: dense (data type: float) is required but could not be found"),
    ({"dense": [0.5] * 13, "sparse": [0] * (T_SPARSE - 1)}, f"values size: {T_SPARSE - 1} but output shape: [{T_SPARSE}]"),
    ({"dense": [0.5] * 12, "sparse": [0] * T_SPARSE}, "values size: 12 but output shape: [13]"),
    ({"dense": [1] * 13, "sparse": [0] * T_SPARSE}, "data type mismatch (expected float)"),
])
def test_parse_example_errors(server, example, message):
    async def go():
        for sig, call in (("classify", "classify"), ("regress", "regress")):
            c = await client(server.port, sig)
            with pytest.raises(TFServingError) as ei:
                await getattr(c, call)("dlrm", example)
            assert ei.value.code == grpc.StatusCode.INVALID_ARGUMENT
            assert message in str(ei.value)
    run(go())


def test_out_of_range_id_is_an_invalid_argument(server):
    dense, sparse = inputs(2)
    sparse[1, 0] = 5          # table 0 has 5 rows

    async def go():
        c = await client(server.port)
        with pytest.raises(TFServingError) as ei:
            await c.predict_tensors("dlrm", {"dense": dense, "sparse": sparse})
        assert ei.value.code == grpc.StatusCode.INVALID_ARGUMENT and "out of range [0, 5)" in str(ei.value)
    run(go())
