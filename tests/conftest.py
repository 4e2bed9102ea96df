import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")


@pytest.fixture(scope="session")
def oracle():
    import itm_testlib
    return itm_testlib.oracle_backend()


@pytest.fixture(scope="session")
def reference_records():
    import itm_testlib
    records = itm_testlib.ReferenceRecords()
    yield records
    records.save()


@pytest.fixture
def ref(request, reference_records):
    """The reference where its build exists, else its record (tests/golden/reference_records.json): see itm_testlib.ReferenceCheck."""
    import itm_testlib
    test_id = f"{request.node.module.__name__}::{request.node.name}"
    return itm_testlib.ReferenceCheck(reference_records, test_id, itm_testlib.reference_backend())


@pytest.fixture(scope="session")
def hip():
    import itm_testlib
    return itm_testlib.hip_backend()


@pytest.fixture(scope="session")
def hip_host():
    """The product library for its host-only entry points (file formats); loads without a GPU."""
    import itm_testlib
    return itm_testlib.hip_backend()
