"""The soak of test_gpu_rvo_env.py with the CPU backend on both sides: it holds the host loops inside the env to the Python model."""
import host_build
import rvo_env_cases as EC

pytestmark = host_build.needs_fma('numpy takes non-FMA norm / matmul variants on this CPU')


def test_soak_model_and_host_loops(pkg):
    from rvo_backend import OracleRvoBackend
    EC.soak(pkg, OracleRvoBackend(), OracleRvoBackend(), B=3, T=8)
