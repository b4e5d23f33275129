import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def pytest_configure(config):
    config.addinivalue_line(
        "markers", "gpu: test requires an MI355X GPU (run via gpurun)")


def pytest_collection_modifyitems(config, items):
    # Nothing needed: -m "not gpu" / -m gpu filtering is done by the driver.
    pass


@pytest.fixture(autouse=True, scope="session")
def _app_base_dir(tmp_path_factory):
    """Launched applications keep their working dirs under pytest's own
    temp dir (the launcher's default is a fixed, shared directory that
    another user's earlier run may own)."""
    if "MIYARN_APP_BASE_DIR" in os.environ:
        yield
        return
    os.environ["MIYARN_APP_BASE_DIR"] = str(
        tmp_path_factory.mktemp("miyarn_apps"))
    yield
    del os.environ["MIYARN_APP_BASE_DIR"]


@pytest.fixture
def kv_server():
    from tf_yarn_amd.kv import KVServer
    server = KVServer()
    yield server
    server.stop()


@pytest.fixture
def kv_client(kv_server):
    from tf_yarn_amd.kv import KVClient
    client = KVClient(kv_server.address)
    yield client
    client.close()
