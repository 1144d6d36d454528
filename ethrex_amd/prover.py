"""Host-side mirror of ethrex's prover backend boundary and pull loop.

The reference host for this path is Rust:
  - trait ProverBackend (crates/prover/src/backend/mod.rs:87-153):
    prover_type / serialize_input / execute / prove(input, format) /
    verify / to_proof_bytes (+ *_timed defaults)
  - pull loop (crates/prover/src/prover.rs:86-140): poll coordinator ->
    InputRequest -> prove -> ProofSubmit, errors continue to next endpoint
  - BackendType registry (mod.rs:49-80)

This module mirrors that interface in Python above the C-ABI (the Rust
binding a maintainer would add instead is in INTEGRATION.md).  Two backends:

  Mi355Backend — the product: drives the gfx950 MSM/NTT core through
    libethrex_mi355.so.  Requires a GPU; fails loudly without one.
  ExecBackend  — the reference's own mock-prover shape
    (crates/prover/src/backend/exec.rs:12-94): executes the statement on
    CPU, emits the sentinel proof bytes (exec.rs:53-60).  Used for
    CPU-only plumbing tests exactly as the reference's CI uses Exec.
"""
import hashlib
import json
import socket
import time


class BackendError(Exception):
    """Mirror of crates/prover/src/backend/error.rs BackendError."""


# ---- ProverOutput / ProofBytes wire shapes (crates/common/types/prover.rs) ----

def proof_output(prover_type: str, proof_bytes: bytes) -> dict:
    return {"Proof": {"prover_type": prover_type,
                      "proof": list(proof_bytes)}}


def _witness_of(input_data):
    """ProgramInput carrying an execution witness: {"witness": {"state":
    [hex], "headers": [hex]}, "first_block_number": N} (the RpcExecution-
    Witness shape of the reference's prover cache fixtures,
    tooling/zkevm_bench/src/cache.rs).  Returns (state, headers, fbn) or
    None for witness-less plumbing inputs."""
    if not (isinstance(input_data, dict) and "witness" in input_data):
        return None
    w = input_data["witness"]

    def _hx(s):
        return bytes.fromhex(s[2:] if s.startswith("0x") else s)
    return ([_hx(s) for s in w["state"]], [_hx(s) for s in w["headers"]],
            int(input_data["first_block_number"]))


class ExecBackend:
    """Mirror of ExecBackend (backend/exec.rs): statement execution on the
    CPU (the reference's Exec path IS a CPU re-execution), sentinel proof
    bytes; the protocol-level mock prover.  Witness-carrying inputs run
    the witness-validation statement (ethrex_amd/witness.py)."""

    def prover_type(self) -> str:
        return "Exec"

    def serialize_input(self, input_data) -> bytes:
        return json.dumps(input_data, sort_keys=True).encode()

    def execute(self, input_data):
        wit = _witness_of(input_data)
        if wit is None:
            self.serialize_input(input_data)  # witness-less plumbing input
            return None
        from . import witness as W
        return W.validate_witness(wit[0], wit[1], wit[2], W.cpu_hash_batch)

    def prove(self, input_data, proof_format: str):
        statement = self.execute(input_data)
        out = {"output": hashlib.sha256(
            self.serialize_input(input_data)).hexdigest()}
        if statement is not None:
            out["statement"] = statement
        return out

    def verify(self, proof) -> None:
        if "output" not in proof:
            raise BackendError("exec: missing output")

    def to_proof_bytes(self, proof, proof_format: str) -> dict:
        # non-empty sentinel (exec.rs:53-60)
        return proof_output("Exec", b"\x00")


class Mi355Backend:
    """The MI355X backend.  `execute` validates the witness (GPU batched
    keccak + trie linking -> statement); `prove` runs the WRAP-SHAPED
    composition the Groth16 wrap performs (backend/sp1.rs:122-134): the
    statement-seeded witness vector is NTT'd and its output feeds the
    proving MSM on device.  Proof bytes = MSM affine result || NTT output
    digest || statement commitment (the wrap circuit itself lives in the
    non-vendored zkVM — SURVEY.md §8c — so the proof-OBJECT is this
    core's composition output, carried through the §8f row-3 wire)."""

    BINDINGS = ("seed", "witness")
    COMPOSITIONS = ("direct", "quotient", "r1cs")
    # composition="r1cs": product-chain circuit v1 (ethrex_amd/r1cs.py) with
    # n constraints, 64 free inputs, 3 entries per A/B row, this circuit seed
    R1CS_K = 64
    R1CS_FAN_IN = 3
    R1CS_SEED = 0x72316373   # "r1cs"

    def __init__(self, msm_log2=16, ntt_log2=12, device=0, binding="seed",
                 composition="direct"):
        # binding: how the composition's input vector is derived.
        #   "seed"    — gen_fr over the first 8 bytes of the statement
        #               commitment (host-generated, uploaded);
        #   "witness" — wrap vector v1 (witness.wrap_vector): expanded on
        #               device from EVERY witness node digest, so any node
        #               byte changes the proof.  Witness-less inputs have
        #               no digests and keep the seed path.
        if binding not in self.BINDINGS:
            raise BackendError(f"mi355: unknown binding {binding!r} "
                               f"(expected one of {self.BINDINGS})")
        # composition: what feeds the proving MSM.
        #   "direct"   — the forward NTT of the input vector;
        #   "quotient" — the Groth16 data flow: two input vectors a, b,
        #                c = a (.) b on device, and the quotient polynomial
        #                h = (A*B - C) / (X^n - 1) (QuotPlan; DESIGN.md
        #                "Quotient polynomial") is the MSM's scalar vector.
        #   "r1cs"     — a satisfied constraint system end to end: the
        #                first 64 elements of the input vector are the free
        #                inputs of product-chain circuit v1, a = A z, b = B z,
        #                c = C z are evaluated on device (R1csPlan) and feed
        #                the quotient, whose h is the MSM's scalar vector.
        if composition not in self.COMPOSITIONS:
            raise BackendError(f"mi355: unknown composition {composition!r} "
                               f"(expected one of {self.COMPOSITIONS})")
        self.msm_log2 = msm_log2
        self.ntt_log2 = ntt_log2
        self.device = device
        self.binding = binding
        self.composition = composition

    def prover_type(self) -> str:
        # reuses Exec semantics for coordinator keying (no on-chain
        # verifier), per SURVEY.md §8b registration nuance
        return "Exec"

    def serialize_input(self, input_data) -> bytes:
        return json.dumps(input_data, sort_keys=True).encode()

    def _seed(self, input_data) -> int:
        return int.from_bytes(
            hashlib.sha256(self.serialize_input(input_data)).digest()[:8],
            "little")

    def _gpu_hash_batch(self, msgs, keep=None):
        """batched keccak over the device KeccakPlan (the witness nodes'
        bulk hashing — §8f row 4).  With a `keep` list the plan is appended
        to it instead of destroyed: its device-resident digests feed the
        witness binding (the caller destroys it)."""
        import ethrex_amd as ea
        offs = [0]
        buf = bytearray()
        for m in msgs:
            buf += m
            offs.append(len(buf))
        kp = ea.KeccakPlan(max(len(buf), 1), len(msgs))
        try:
            kp.upload(bytes(buf), offs)
            kp.run()
            out = kp.download()
        except BaseException:
            kp.destroy()
            raise
        if keep is None:
            kp.destroy()
        else:
            keep.append(kp)
        return [out[32 * i:32 * i + 32] for i in range(len(msgs))]

    def execute(self, input_data):
        """The witness-validation statement, with the node hashing on the
        GPU (block_execution_witness.rs rebuild semantics); witness-less
        plumbing inputs keep the serialize-only behavior."""
        return self._execute(input_data, None)

    def _execute(self, input_data, keep):
        wit = _witness_of(input_data)
        if wit is None:
            self.serialize_input(input_data)
            return None
        import ethrex_amd as ea
        if ea.device_count() < 1:
            raise BackendError("mi355: no GPU visible (no CPU fallback)")
        ea.set_device(self.device)
        from . import witness as W
        return W.validate_witness(
            wit[0], wit[1], wit[2],
            lambda msgs: self._gpu_hash_batch(msgs, keep))

    def prove(self, input_data, proof_format: str):
        import ethrex_amd as ea
        if ea.device_count() < 1:
            raise BackendError("mi355: no GPU visible (no CPU fallback)")
        ea.set_device(self.device)
        kplans = [] if self.binding == "witness" else None
        try:
            statement = self._execute(input_data, kplans)
        except BaseException:
            for kp in kplans or ():
                kp.destroy()
            raise
        if statement is not None:
            # the proof binds to the STATEMENT (initial state root +
            # linked-witness commitment), not to a hash of the input JSON
            seed = int.from_bytes(
                bytes.fromhex(statement["commitment"])[:8], "little")
        else:
            seed = self._seed(input_data)
        # the wrap-shaped composition (backend/sp1.rs:122-134 flow): the
        # statement-derived witness vector is NTT'd and its output feeds
        # the proving MSM ON DEVICE (msm_scalars_from_ntt) — the two
        # primitives this core exists for, composed as the Groth16 wrap
        # composes them, with no PCIe hop between them.
        n = 1 << self.msm_log2
        if self.composition in ("quotient", "r1cs"):
            run = (self._prove_quotient if self.composition == "quotient"
                   else self._prove_r1cs)
            try:
                msm_out, ntt_out = run(ea, n, seed, statement, kplans)
            finally:
                for kp in kplans or ():
                    kp.destroy()
            proof = {"msm": msm_out,
                     "ntt_digest": hashlib.sha256(ntt_out).digest()}
            if statement is not None:
                proof["statement"] = statement
            return proof
        plan = ea.MsmPlan(n)
        nplan = ea.NttPlan(n)
        try:
            plan.gen_points(0)
            if kplans:
                # witness binding: the statement pass hashed every state
                # node in ONE batch, whose digests are still in HBM
                nplan.fill_from_digests(
                    kplans[-1], bytes.fromhex(statement["commitment"]))
            else:
                nplan.upload(ea.gen_fr(seed, n))
            nplan.run(False)
            plan.scalars_from_ntt(nplan, 0)
            msm_out = plan.run()
            ntt_out = nplan.download()
        finally:
            plan.destroy()
            nplan.destroy()
            for kp in kplans or ():
                kp.destroy()
        proof = {"msm": msm_out,
                 "ntt_digest": hashlib.sha256(ntt_out).digest()}
        if statement is not None:
            proof["statement"] = statement
        return proof

    def _prove_quotient(self, ea, n, seed, statement, kplans):
        """composition="quotient": a, b -> c = a (.) b -> h on device, h
        feeds the MSM through the same on-device handoff.  Returns (MSM
        result, h bytes)."""
        from . import witness as W
        plan = ea.MsmPlan(n)
        qplan = ea.QuotPlan(n)
        nplan = None
        try:
            plan.gen_points(0)
            if kplans:
                commitment = bytes.fromhex(statement["commitment"])
                nplan = ea.NttPlan(n)
                nplan.fill_from_digests(kplans[-1], commitment)
                qplan.load_from_ntt(0, nplan)
                nplan.fill_from_digests(kplans[-1],
                                        W.quotient_domain_b(commitment))
                qplan.load_from_ntt(1, nplan)
            else:
                qplan.upload(0, ea.gen_fr(seed, n))
                qplan.upload(1, ea.gen_fr((seed + 1) % (1 << 64), n))
            qplan.mul_ab_into_c()
            qplan.run()
            plan.scalars_from_ntt(qplan, 0)
            return plan.run(), qplan.download()
        finally:
            plan.destroy()
            qplan.destroy()
            if nplan is not None:
                nplan.destroy()

    def _prove_r1cs(self, ea, n, seed, statement, kplans):
        """composition="r1cs": z on the host from 64 free inputs, A z, B z,
        C z on device, device-to-device into the quotient, h feeds the MSM.
        Returns (MSM result, h bytes)."""
        from . import r1cs as C
        k = self.R1CS_K
        if n < k:
            raise BackendError("mi355: composition r1cs needs msm_log2 >= 6")
        if kplans:
            nplan = ea.NttPlan(n)
            try:
                nplan.fill_from_digests(
                    kplans[-1], bytes.fromhex(statement["commitment"]))
                free = nplan.download()[:32 * k]
            finally:
                nplan.destroy()
        else:
            free = ea.gen_fr(seed, k)
        mats, witness = C.chain_circuit(n, k, self.R1CS_FAN_IN,
                                        self.R1CS_SEED)
        z = witness([int.from_bytes(free[32 * i:32 * i + 32], "big")
                     for i in range(k)])
        plan = ea.MsmPlan(n)
        qplan = ea.QuotPlan(n)
        rplan = ea.R1csPlan(n, len(z))
        try:
            plan.gen_points(0)
            for which, (offs, cols, coeffs) in enumerate(mats):
                rplan.upload_matrix(which, offs, cols, C.fr_bytes(coeffs))
            rplan.upload_witness(C.fr_bytes(z))
            rplan.eval_all()
            for which in range(3):
                qplan.load_from_r1cs(which, rplan, which)
            qplan.run()
            plan.scalars_from_ntt(qplan, 0)
            return plan.run(), qplan.download()
        finally:
            plan.destroy()
            qplan.destroy()
            rplan.destroy()

    def verify(self, proof) -> None:
        if len(proof.get("msm", b"")) != 64:
            raise BackendError("mi355: bad proof")

    def to_proof_bytes(self, proof, proof_format: str) -> dict:
        pb = proof["msm"] + proof["ntt_digest"]
        if "statement" in proof:
            pb += bytes.fromhex(proof["statement"]["commitment"])
        return proof_output(self.prover_type(), pb)


BACKENDS = {"exec": ExecBackend, "mi355": Mi355Backend}


# ---- pull-loop client (crates/prover/src/prover.rs:86-198,289-305) ----

def _round_trip(host, port, obj, timeout=10.0):
    with socket.create_connection((host, port), timeout=timeout) as conn:
        conn.sendall(json.dumps(obj).encode())
        conn.shutdown(socket.SHUT_WR)
        chunks = []
        while True:
            b = conn.recv(65536)
            if not b:
                break
            chunks.append(b)
    return json.loads(b"".join(chunks).decode()) if chunks else None


class ProverClient:
    def __init__(self, backend, endpoints, commit_hash="deadbeef",
                 proving_interval_s=0.05):
        self.backend = backend
        self.endpoints = endpoints  # [(host, port)]
        self.commit_hash = commit_hash
        self.interval = proving_interval_s
        self.proved = []

    def poll_once(self) -> int:
        """One pass over all endpoints (poll_endpoints, prover.rs:86-140).
        Returns number of proofs submitted; errors continue to the next
        endpoint (prover.rs:100-103,129-138)."""
        done = 0
        for (host, port) in self.endpoints:
            try:
                resp = _round_trip(host, port, {"InputRequest": {
                    "commit_hash": self.commit_hash,
                    "prover_type": self.backend.prover_type()}})
                if resp == "VersionMismatch":
                    raise BackendError("version mismatch with coordinator")
                if not (isinstance(resp, dict) and "InputResponse" in resp):
                    continue
                ir = resp["InputResponse"]
                if ir.get("id") is None:
                    continue  # no work available
                proof = self.backend.prove(ir["input"], ir.get("format"))
                self.backend.verify(proof)
                out = self.backend.to_proof_bytes(proof, ir.get("format"))
                ack = _round_trip(host, port, {"ProofSubmit": {
                    "id": ir["id"], "proof": out}})
                if isinstance(ack, dict) and "ProofSubmitACK" in ack:
                    self.proved.append(ir["id"])
                    done += 1
            except BackendError:
                raise
            except (OSError, json.JSONDecodeError):
                continue  # endpoint error: move on (prover.rs:100-103)
        return done

    def run(self, max_polls=100):
        """Re-scheduling poll loop (Handler<Poll>, prover.rs:214-222)."""
        for _ in range(max_polls):
            if self.poll_once() == 0:
                time.sleep(self.interval)
        return self.proved
