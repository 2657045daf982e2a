"""ComposableResource controller: the per-device 5-state machine.

State-machine parity with the reference
(composableresource_controller.go:106-434):

    "" → Attaching → Online → Detaching → Deleting

with the amdgpu/CDI node path substituted and one deliberate
performance departure: where the reference re-queues on fixed 30 s / 3 s
intervals while waiting for hardware (``:236,298,330,400``), this build uses
sub-second configurable waits (``ReconcileConfig``) — hardware readiness is
bounded by the PCIe rescan + amdgpu bind time, not by a poll quantum.  That
is the p50 attach→CDI-ready win BASELINE.md targets.

Additions over the reference on the Online transition:
* the CDI spec is written (north-star requirement — the reference delegates
  device exposure to the NVIDIA plugin stack);
* an optional gfx950 health probe (HIP MFMA + HBM kernel) validates the
  composed device actually computes before it is advertised;
* ``cro_attach_to_ready_seconds`` is observed.
"""

from __future__ import annotations

import logging
import time
from dataclasses import dataclass
from typing import Dict, Optional

from ..api.v1alpha1.types import ComposableResource
from ..fabric import Adapter, FabricError, WaitingDeviceAttaching, WaitingDeviceDetaching
from ..metrics import Metrics
from ..nodeops import amdgpu, taints
from ..nodeops.amdgpu import GPULoadsPresent, ScrubFailed
from ..nodeops.nodes import node_exists
from ..runtime.client import Client
from ..runtime.controller import Reconciler, Result
from ..runtime.errors import ConflictError, NotFoundError
from ..runtime.store import _now_rfc3339

log = logging.getLogger(__name__)

FINALIZER = "cro.amd.com/finalizer"
READY_TO_DETACH_LABEL = "cro.amd.com/ready-to-detach-device-id"
READY_TO_DETACH_CDI_LABEL = "cro.amd.com/ready-to-detach-cdi-device-id"
MANAGED_BY_LABEL = "app.kubernetes.io/managed-by"


@dataclass
class ReconcileConfig:
    # wait for device visibility after fabric attach (reference: 30 s)
    attach_visible_wait: float = 0.05
    # waits while the fabric reports attach/detach in progress
    # (reference: fixed 30 s): exponential from base to max so attach
    # tracks the fabric's actual compose time + a bounded overshoot
    # instead of quantizing to a fixed poll step
    fabric_wait_base: float = 0.05
    fabric_wait_max: float = 1.0
    # Online health-check period (reference: 30 s — not latency-critical)
    online_health_period: float = 30.0
    # wait for device invisibility during detach (reference: 3 s)
    detach_invisible_wait: float = 0.05


class ComposableResourceReconciler(Reconciler):
    def __init__(
        self,
        client: Client,
        adapter: Adapter,
        node_ops: amdgpu.NodeOps,
        config: Optional[ReconcileConfig] = None,
        recorder=None,
    ):
        from ..runtime.events import NullRecorder

        self.client = client
        self.adapter = adapter
        self.node_ops = node_ops
        self.config = config or ReconcileConfig()
        self.recorder = recorder or NullRecorder()
        self.metrics = Metrics()
        # uid → monotonic time of Attaching entry (restart loses the sample,
        # never corrupts it — the histogram only sees fully observed attaches)
        self._attach_started: Dict[str, float] = {}
        self._detach_started: Dict[str, float] = {}
        # uids whose device passed its scrub in this detach: the handler is
        # re-entered on every fabric wait and drain poll, and a device that is
        # mid-removal must not be scrubbed again
        self._scrub_done: Dict[str, bool] = {}
        # uid → consecutive fabric-waiting polls (for the exponential wait)
        self._fabric_polls: Dict[str, int] = {}

    # -- plumbing ----------------------------------------------------------

    def reconcile(self, name: str) -> Result:
        try:
            resource = self.client.get(ComposableResource, name)
        except NotFoundError:
            return Result()

        if self._garbage_collect(resource):
            return Result()

        state = resource.status.state
        handler = {
            "": self._handle_none,
            "Attaching": self._handle_attaching,
            "Online": self._handle_online,
            "Detaching": self._handle_detaching,
            "Deleting": self._handle_deleting,
        }.get(state)
        if handler is None:
            return Result()  # unknown state: parity with reference default (no-op)
        try:
            return handler(resource)
        except ConflictError:
            raise  # retry with fresh read; no status scribbling on conflicts
        except Exception as exc:
            self._set_error(resource, str(exc))
            raise

    def _restart_plugin_daemonsets(
        self, resource: ComposableResource, fatal: bool
    ) -> ComposableResource:
        """DEVICE_PLUGIN node refresh: roll the AMD device-plugin and
        metrics-exporter daemonsets (nvidia-device-plugin-daemonset +
        nvidia-dcgm parity, composableresource_controller.go:257-269).

        Daemonsets not present in the store mean this deployment does not
        model them (standalone single-node) — skipped, not an error; a
        present daemonset that fails to update is surfaced per the
        reference's attach (log) / detach (fatal) split.
        """
        import os

        from ..nodeops.nodes import restart_daemonset

        namespace = os.environ.get("CRO_AMD_GPU_OPERATOR_NAMESPACE", "amd-gpu-operator")
        for name in ("amd-device-plugin", "amd-metrics-exporter"):
            try:
                restart_daemonset(self.client, namespace, name)
            except NotFoundError:
                log.debug("daemonset %s/%s not modeled; skipping restart", namespace, name)
            except Exception as exc:
                if fatal:
                    raise
                log.warning("failed to restart %s/%s: %s", namespace, name, exc)
                resource.status.error = str(exc)
                try:
                    # keep the fresh resourceVersion so the caller's next
                    # status write does not conflict pointlessly
                    resource = self.client.update_status(resource)
                except ConflictError:
                    pass
        return resource

    def _fabric_wait(self, resource: ComposableResource) -> float:
        """Exponential wait between async-fabric polls, resumable across
        operator restarts: the first Waiting persists
        ``status.fabric_wait_started``; a restarted operator (empty
        in-memory counter, timestamp set) resumes directly at the max
        interval instead of re-ramping from the base — an async fabric
        mid-compose is never hammered after a failover (VERDICT r1
        weak #5)."""
        uid = resource.metadata.uid
        n = self._fabric_polls.get(uid, 0)
        if n == 0 and resource.status.fabric_wait_started:
            # restart mid-wait: skip the ramp entirely
            self._fabric_polls[uid] = 17
            return self.config.fabric_wait_max
        self._fabric_polls[uid] = n + 1
        wait = min(self.config.fabric_wait_base * (2 ** min(n, 16)),
                   self.config.fabric_wait_max)
        # Persist the marker only once the ramp hits its cap: short composes
        # finish before this and keep a write-free poll schedule (a status
        # write would requeue us immediately and skew the ramp); a compose
        # still pending at the cap is the long-running case where restart
        # resumption matters.
        if wait >= self.config.fabric_wait_max and not resource.status.fabric_wait_started:
            resource.status.fabric_wait_started = _now_rfc3339()
            try:
                self.client.update_status(resource)
            except ConflictError:
                pass  # a racing write wins; next poll persists again
        return wait

    def _persist_device_identity(
        self, name: str, device_id: str, cdi_device_id: str
    ) -> ComposableResource:
        last_exc = None
        for _ in range(8):
            try:
                fresh = self.client.get(ComposableResource, name)
                fresh.status.error = ""
                fresh.status.device_id = device_id
                fresh.status.cdi_device_id = cdi_device_id
                fresh.status.fabric_wait_started = ""  # wait concluded
                return self.client.update_status(fresh)
            except ConflictError as exc:
                last_exc = exc
        raise last_exc

    def _phase(self, name: str):
        """Attach-phase span recorded into cro_attach_phase_seconds."""
        import contextlib

        @contextlib.contextmanager
        def span():
            t0 = time.monotonic()
            try:
                yield
            finally:
                self.metrics.attach_phase_seconds.labels(name).observe(
                    time.monotonic() - t0
                )

        return span()

    def _scrub_before_drain(self, resource: ComposableResource, ops) -> None:
        """Overwrite and verify the device's VRAM (and, where the scrub hook
        covers them, every CU's LDS and every SIMD's vector registers: the
        result then has an "lds" and a "regs" object) before it leaves the
        node, once per detach.  A scrub that does not pass keeps
        the device here (ScrubFailed) unless the detach is forced."""
        uid = resource.metadata.uid
        if self._scrub_done.get(uid):
            return
        device_id = resource.status.device_id
        t0 = time.monotonic()
        try:
            result = ops.scrub(resource.spec.target_node, device_id)
        except Exception as exc:  # a scrub that could not run is a failed scrub
            result = {"ok": False, "rc": -1, "msg": f"{type(exc).__name__}: {exc}"}
        if result is None:
            return  # not configured, or the device is already off the node
        # the "scrub" phase, recorded only when a scrub ran: with the feature
        # off the phase histogram keeps exactly the labels it had
        elapsed = time.monotonic() - t0
        self.metrics.attach_phase_seconds.labels("scrub").observe(elapsed)
        self.metrics.scrub_seconds.observe(elapsed)
        scrubbed = int(result.get("bytes_scrubbed", 0) or 0)
        self.metrics.scrub_bytes_total.inc(scrubbed)
        fraction = float(result.get("fraction", 0.0) or 0.0)
        lds = result.get("lds") if isinstance(result.get("lds"), dict) else None
        regs = result.get("regs") if isinstance(result.get("regs"), dict) else None
        if result.get("ok"):
            self._scrub_done[uid] = True
            lds_clause = ""
            if lds is not None:
                lds_clause = (
                    f"; LDS of {int(lds.get('cus_seen', 0) or 0)} of "
                    f"{int(lds.get('cus_expected', 0) or 0)} CUs cleared "
                    f"({int(lds.get('bytes_scrubbed', 0) or 0) // 1024} KiB), "
                    f"{int(lds.get('dirty_words_before', 0) or 0)} dirty LDS words found before"
                )
            regs_clause = ""
            if regs is not None:
                regs_clause = (
                    f"; vector registers of {int(regs.get('simds_seen', 0) or 0)} of "
                    f"{int(regs.get('simds_expected', 0) or 0)} SIMDs cleared "
                    f"({int(regs.get('bytes_scrubbed', 0) or 0) // 1024} KiB), "
                    f"{int(regs.get('dirty_words_before', 0) or 0)} dirty register words "
                    "found before"
                )
            self.recorder.normal(
                resource,
                "Scrubbed",
                f"scrubbed {scrubbed / 2**30:.2f} GiB ({100.0 * fraction:.1f} % of VRAM) "
                f"of device {device_id}, verified; "
                f"{int(result.get('dirty_words_before', 0) or 0)} dirty words found before; "
                f"{float(result.get('t_total_ms', 0.0) or 0.0):.0f} ms" + lds_clause + regs_clause,
            )
            return
        reason = {
            -40: "residue", -41: "fraction", -42: "lds_residue", -43: "lds_coverage",
            -44: "reg_residue", -45: "reg_coverage",
        }.get(result.get("rc"), "error")
        self.metrics.scrub_failures_total.labels(reason=reason).inc()
        # lead with what an operator acts on, before the scrub's own message
        if reason in ("lds_residue", "lds_coverage"):
            where = lds if lds is not None else result
            msg = (
                f"scrub of device {device_id} failed: {reason} "
                f"xcd={where.get('xcd')} se={where.get('se')} sh={where.get('sh')} "
                f"cu={where.get('cu')} first_bad_word={where.get('first_bad_word')} "
                f"bits_bad=0x{int(where.get('bits_bad', 0) or 0):08x} "
                f"n_bad={where.get('n_bad')} "
                f"recheck_dirty_words={where.get('recheck_dirty_words')} "
                f"cus_seen={where.get('cus_seen')}/{where.get('cus_expected')}: "
                f"{result.get('msg', '')}"
            )
        elif reason in ("reg_residue", "reg_coverage"):
            where = regs if regs is not None else result
            msg = (
                f"scrub of device {device_id} failed: {reason} "
                f"xcd={where.get('xcd')} se={where.get('se')} sh={where.get('sh')} "
                f"cu={where.get('cu')} simd={where.get('simd')} wave={where.get('wave')} "
                f"first_bad_word={where.get('first_bad_word')} "
                f"bits_bad=0x{int(where.get('bits_bad', 0) or 0):08x} "
                f"n_bad={where.get('n_bad')} "
                f"recheck_dirty_words={where.get('recheck_dirty_words')} "
                f"simds_seen={where.get('simds_seen')}/{where.get('simds_expected')}: "
                f"{result.get('msg', '')}"
            )
        else:
            msg = (
                f"scrub of device {device_id} failed: {reason} "
                f"first_bad_byte={result.get('first_bad_byte')} "
                f"bits_bad=0x{int(result.get('bits_bad', 0) or 0):08x} "
                f"n_bad={result.get('n_bad')} fraction={fraction:.4f}: {result.get('msg', '')}"
            )
        if resource.spec.force_detach:
            self.recorder.warning(resource, "ScrubFailed", msg + "; force_detach: detaching anyway")
            self._scrub_done[uid] = True  # force means force, and once
            return
        self.recorder.warning(resource, "ScrubFailed", msg)
        raise ScrubFailed(msg)

    def _set_error(self, resource: ComposableResource, msg: str) -> None:
        """requeueOnErr parity: persist the failure into .status.error
        (composableresource_controller.go:436-446)."""
        try:
            fresh = self.client.get(ComposableResource, resource.metadata.name)
            fresh.status.error = msg
            self.client.update_status(fresh)
        except Exception:
            log.debug("could not record error on %s", resource.metadata.name)
        self.recorder.warning(resource, "ReconcileError", msg)

    def _garbage_collect(self, resource: ComposableResource) -> bool:
        """Target node deleted → taint cleanup, Deleting, delete CR
        (composableresource_controller.go:137-183)."""
        if not resource.spec or not resource.spec.target_node:
            return False
        if node_exists(self.client, resource.spec.target_node):
            return False
        if taints.has_device_taint(self.client, resource):
            taints.delete_device_taint(self.client, resource)
        did = False
        if resource.status.state == "Online":
            self.metrics.devices_online.dec()  # GC skips the Detaching edge
        if resource.status.state != "Deleting":
            resource.status.state = "Deleting"
            resource.status.error = f"target node {resource.spec.target_node} not found"
            resource = self.client.update_status(resource)
            did = True
        if resource.metadata.deletionTimestamp is None:
            self.client.delete(resource)
            did = True
        if did:
            self.recorder.warning(
                resource,
                "GarbageCollected",
                f"target node {resource.spec.target_node} deleted",
            )
        return did

    # -- states ------------------------------------------------------------

    def _handle_none(self, resource: ComposableResource) -> Result:
        if FINALIZER not in resource.metadata.finalizers:
            resource.metadata.finalizers.append(FINALIZER)
            resource = self.client.update(resource)

        # syncer-created detach CRs carry the device identity in labels
        # (upstreamsyncer_controller.go:140-165 → :195-202)
        device_id = resource.metadata.labels.get(READY_TO_DETACH_LABEL, "")
        if device_id:
            resource.status.device_id = device_id
            cdi_id = resource.metadata.labels.get(READY_TO_DETACH_CDI_LABEL, "")
            if cdi_id:
                resource.status.cdi_device_id = cdi_id

        self._attach_started[resource.metadata.uid] = time.monotonic()
        resource.status.state = "Attaching"
        resource.status.error = ""
        self.client.update_status(resource)
        self.recorder.normal(
            resource,
            "AttachStarted",
            f"attaching {resource.spec.type}/{resource.spec.model} "
            f"on {resource.spec.target_node}",
        )
        return Result()

    def _handle_attaching(self, resource: ComposableResource) -> Result:
        if resource.metadata.deletionTimestamp is not None:
            if resource.status.device_id == "":
                resource.status.state = "Deleting"
                self.client.update_status(resource)
                return Result()
            elif resource.status.error != "":
                resource.status.state = "Detaching"
                self.client.update_status(resource)
                return Result()

        node = resource.spec.target_node
        mode = self.adapter.device_resource_type
        ops = self.node_ops.for_type(resource.spec.type)

        with self._phase("driver_gate"):
            ops.ensure_driver(node)

        if resource.status.device_id == "":
            t0 = time.monotonic()
            try:
                device_id, cdi_device_id = self.adapter.provider.add_resource(resource)
            except WaitingDeviceAttaching:
                return Result(requeue_after=self._fabric_wait(resource))
            finally:
                self.metrics.fabric_request_seconds.labels(
                    self.adapter.provider.name, "add"
                ).observe(time.monotonic() - t0)
            # Fabric sanity: a buggy/poisoned fabric manager handing out a
            # device some other CR already claims would silently dual-map
            # one GPU into two workloads (the reference has no such guard)
            for other in self.client.list(ComposableResource, copy=False):
                if (
                    other.metadata.name != resource.metadata.name
                    and other.status.device_id == device_id
                ):
                    raise FabricError(
                        f"fabric returned device {device_id} already claimed "
                        f"by {other.metadata.name}; refusing dual attachment"
                    )
            # Persist the fabric-assigned identity with conflict-retry: a
            # concurrent deletion bumps the RV, and dropping this write
            # would leak the attached device (the CR would reach Deleting
            # with device_id "" while the fabric holds the attachment —
            # the upstream syncer would only repair it after the grace
            # period).  The identity is correct regardless of what raced.
            resource = self._persist_device_identity(
                resource.metadata.name, device_id, cdi_device_id
            )
            self._fabric_polls.pop(resource.metadata.uid, None)
            self.recorder.normal(
                resource, "FabricAttached", f"fabric composed device {device_id}"
            )

        if mode == "DEVICE_PLUGIN":
            # load check is advisory on attach (reference logs and continues,
            # composableresource_controller.go:253-256)
            try:
                ops.check_no_loads(node)
            except GPULoadsPresent as exc:
                log.warning("gpu loads during attach on %s: %s", node, exc)
            resource = self._restart_plugin_daemonsets(resource, fatal=False)
        with self._phase("node_refresh"):
            ops.refresh_after_attach(node)

        if mode == "DRA":
            visible = ops.is_visible_dra(node, resource.status.device_id)
        else:
            visible = ops.is_visible(node, resource.status.device_id)
        if not visible:
            return Result(requeue_after=self.config.attach_visible_wait)

        # device enumerable → emit the Container Device Interface spec and
        # (optionally) verify compute.  NOTE: status.cdi_device_id is the
        # *Composable Disaggregated Infrastructure* id the fabric handed out
        # (FM detach keys on it, fm/client.go:231-242) — the container-CDI
        # spec name is amd.com/gpu=<device_id>, never stored over it.
        with self._phase("cdi_write"):
            ops.write_cdi(node, resource.status.device_id)
        with self._phase("health_probe"):
            probe = ops.health_probe(node, resource.status.device_id)
        if probe is not None and not probe.get("ok", True):
            compute = probe.get("compute")
            if isinstance(compute, dict) and not compute.get("ok", True):
                # compute stage: lead with the check and where on the chip it
                # failed — what an RMA or a CU mask needs — before the raw dict
                test = compute.get("failed_test") or (
                    "coverage" if compute.get("rc") == -31 else "unknown"
                )
                self.metrics.probe_compute_failures_total.labels(test=test).inc()
                raise FabricError(
                    "gfx950 health probe failed: compute stage "
                    f"{test} xcd={compute.get('xcd')} se={compute.get('se')} "
                    f"cu={compute.get('cu')} simd={compute.get('simd')} "
                    f"bits_bad=0x{int(compute.get('bits_bad', 0)):08x} "
                    f"cus_bad={compute.get('cus_bad')}: {probe}"
                )
            formats = probe.get("formats")
            if isinstance(formats, dict) and not formats.get("ok", True):
                # matrix-format stage: the same lead as the compute stage's
                test = formats.get("failed_test") or (
                    "coverage" if formats.get("rc") == -33 else "unknown"
                )
                self.metrics.probe_formats_failures_total.labels(test=test).inc()
                raise FabricError(
                    "gfx950 health probe failed: formats stage "
                    f"{test} xcd={formats.get('xcd')} se={formats.get('se')} "
                    f"cu={formats.get('cu')} simd={formats.get('simd')} "
                    f"bits_bad=0x{int(formats.get('bits_bad', 0)):08x} "
                    f"cus_bad={formats.get('cus_bad')}: {probe}"
                )
            coherence = probe.get("coherence")
            if isinstance(coherence, dict) and not coherence.get("ok", True):
                # coherence stage: the check, then where: the place of a wave
                # or a workgroup line, or the tally line and slot
                test = coherence.get("failed_test") or (
                    "coverage" if coherence.get("rc") == -35 else "unknown"
                )
                self.metrics.probe_coherence_failures_total.labels(test=test).inc()
                where = (
                    f"xcd={coherence.get('xcd')} se={coherence.get('se')} "
                    f"cu={coherence.get('cu')} simd={coherence.get('simd')}"
                )
                level = coherence.get("tally_level", -1)
                if isinstance(level, int) and 0 <= level <= 2:
                    where += (
                        f" level={('workgroup', 'xcd', 'device')[level]}"
                        f" line={coherence.get('tally_unit')} slot={coherence.get('tally_slot')}"
                        f" got=0x{int(coherence.get('tally_got', 0)):x}"
                        f" want=0x{int(coherence.get('tally_want', 0)):x}"
                    )
                raise FabricError(
                    f"gfx950 health probe failed: coherence stage {test} {where} "
                    f"block={coherence.get('bad_block')} cus_bad={coherence.get('cus_bad')}: {probe}"
                )
            movement = probe.get("movement")
            if isinstance(movement, dict) and not movement.get("ok", True):
                # data-movement stage: the check, which variant, lane and
                # register received the wrong word, then where on the chip
                from ..nodeops.movement import describe_first_bad

                test = movement.get("failed_test") or (
                    "coverage" if movement.get("rc") == -37 else "unknown"
                )
                self.metrics.probe_movement_failures_total.labels(test=test).inc()
                what = ""
                if movement.get("failed_test"):
                    what = describe_first_bad(test, int(movement.get("first_bad", 0))) + " "
                raise FabricError(
                    f"gfx950 health probe failed: movement stage {test} {what}"
                    f"xcd={movement.get('xcd')} se={movement.get('se')} "
                    f"cu={movement.get('cu')} simd={movement.get('simd')} "
                    f"bits_bad=0x{int(movement.get('bits_bad', 0)):08x} "
                    f"cus_bad={movement.get('cus_bad')}: {probe}"
                )
            alu = probe.get("alu")
            if isinstance(alu, dict) and not alu.get("ok", True):
                # ALU stage: the check, which form, row and lane gave the
                # wrong word, then where on the chip
                from ..nodeops.alu import describe_first_bad as describe_alu

                test = alu.get("failed_test") or (
                    "coverage" if alu.get("rc") == -39 else "unknown"
                )
                self.metrics.probe_alu_failures_total.labels(test=test).inc()
                what = ""
                if alu.get("failed_test"):
                    what = describe_alu(int(alu.get("first_bad", 0))) + " "
                raise FabricError(
                    f"gfx950 health probe failed: alu stage {test} {what}"
                    f"xcd={alu.get('xcd')} se={alu.get('se')} "
                    f"cu={alu.get('cu')} simd={alu.get('simd')} "
                    f"bits_bad=0x{int(alu.get('bits_bad', 0)):08x} "
                    f"cus_bad={alu.get('cus_bad')}: {probe}"
                )
            integrity = probe.get("integrity")
            if isinstance(integrity, dict) and not integrity.get("ok", True):
                # deep level: lead with what an operator needs to act on —
                # which stage, where, which bits — before the raw dict
                stage = integrity.get("failed_stage") or "unknown"
                self.metrics.probe_integrity_failures_total.labels(stage=stage).inc()
                raise FabricError(
                    "gfx950 health probe failed: integrity stage "
                    f"{stage} first_bad_byte={integrity.get('first_bad_byte')} "
                    f"bits_bad=0x{int(integrity.get('bits_bad', 0)):08x} "
                    f"n_bad={integrity.get('n_bad')}: {probe}"
                )
            raise FabricError(f"gfx950 health probe failed: {probe}")

        resource.status.state = "Online"
        resource.status.error = ""
        self.client.update_status(resource)
        probe_note = ""
        if probe is not None:
            probe_note = (
                f"; probe: mfma_exact={probe.get('mfma_f32_exact')} "
                f"hbm={probe.get('hbm_gbps', 0):.0f} GB/s"
            )
            compute = probe.get("compute")
            if isinstance(compute, dict):
                probe_note += (
                    f"; compute: {compute.get('cus_seen', 0)}/{compute.get('cus_expected', 0)}"
                    f" CUs, {compute.get('simds_seen', 0)} SIMDs,"
                    f" {compute.get('gpu_ms', 0):.1f} ms"
                )
            formats = probe.get("formats")
            if isinstance(formats, dict):
                probe_note += (
                    f"; formats: {formats.get('cus_seen', 0)}/{formats.get('cus_expected', 0)}"
                    f" CUs, {formats.get('simds_seen', 0)} SIMDs,"
                    f" {formats.get('gpu_ms', 0):.1f} ms"
                )
            coherence = probe.get("coherence")
            if isinstance(coherence, dict):
                probe_note += (
                    f"; coherence: {coherence.get('cus_seen', 0)}"
                    f"/{coherence.get('cus_expected', 0)} CUs,"
                    f" {coherence.get('pairs_checked', 0)} pairs,"
                    f" {coherence.get('gpu_ms', 0):.1f} ms"
                )
            movement = probe.get("movement")
            if isinstance(movement, dict):
                probe_note += (
                    f"; movement: {movement.get('cus_seen', 0)}"
                    f"/{movement.get('cus_expected', 0)} CUs,"
                    f" {movement.get('simds_seen', 0)} SIMDs,"
                    f" {movement.get('gpu_ms', 0):.1f} ms"
                )
            alu = probe.get("alu")
            if isinstance(alu, dict):
                probe_note += (
                    f"; alu: {alu.get('cus_seen', 0)}"
                    f"/{alu.get('cus_expected', 0)} CUs,"
                    f" {alu.get('simds_seen', 0)} SIMDs,"
                    f" {alu.get('gpu_ms', 0):.1f} ms"
                )
            integrity = probe.get("integrity")
            if isinstance(integrity, dict):
                link = min(
                    integrity.get("h2d_dma_bytes_verified", 0),
                    integrity.get("d2h_dma_bytes_verified", 0),
                )
                # span, not span x passes
                vram = integrity.get("vram_bytes_verified", 0) // max(
                    integrity.get("vram_passes", 1), 1
                )
                probe_note += (
                    f"; integrity: vram {vram / 2**30:.2f} GiB"
                    f" link {link / 2**30:.2f} GiB verified,"
                    f" h2d {integrity.get('h2d_dma_gbps', 0):.1f}"
                    f" d2h {integrity.get('d2h_dma_gbps', 0):.1f} GB/s"
                )
        self.recorder.normal(
            resource,
            "Online",
            f"device {resource.status.device_id} online with CDI spec{probe_note}",
        )
        started = self._attach_started.pop(resource.metadata.uid, None)
        if started is not None:
            self.metrics.attach_to_ready_seconds.observe(time.monotonic() - started)
        self.metrics.devices_online.inc()
        return Result()

    def _handle_online(self, resource: ComposableResource) -> Result:
        if resource.metadata.deletionTimestamp is not None:
            self._detach_started[resource.metadata.uid] = time.monotonic()
            resource.status.state = "Detaching"
            self.client.update_status(resource)
            self.metrics.devices_online.dec()
            self.recorder.normal(
                resource,
                "DetachStarted",
                f"detaching device {resource.status.device_id}",
            )
            return Result()

        if resource.metadata.labels.get(READY_TO_DETACH_LABEL, ""):
            # syncer-created CR reached Online bookkeeping: delete to detach
            # (composableresource_controller.go:310-315)
            self.client.delete(resource)
            return Result()

        t0 = time.monotonic()
        try:
            self.adapter.provider.check_resource(resource)
        except FabricError as exc:
            resource.status.error = str(exc)
            self.client.update_status(resource)
            self.recorder.warning(resource, "HealthCheckFailed", str(exc))
            return Result(requeue_after=self.config.online_health_period)
        finally:
            self.metrics.fabric_request_seconds.labels(
                self.adapter.provider.name, "check"
            ).observe(time.monotonic() - t0)
        if resource.status.error:
            resource.status.error = ""
            self.client.update_status(resource)
        return Result(requeue_after=self.config.online_health_period)

    def _handle_detaching(self, resource: ComposableResource) -> Result:
        node = resource.spec.target_node
        mode = self.adapter.device_resource_type
        ops = self.node_ops.for_type(resource.spec.type)

        if resource.status.device_id != "":
            if not resource.spec.force_detach:
                if mode == "DEVICE_PLUGIN":
                    ops.check_no_loads(node)  # whole node
                else:
                    ops.check_no_loads(node, resource.status.device_id)

            if mode == "DRA":
                taints.create_device_taint(self.client, resource)

            self._scrub_before_drain(resource, ops)

            try:
                ops.drain(node, resource.status.device_id)
            except amdgpu.DrainInProgress:
                # last-device drains run asynchronously (module unload can
                # block); poll completion at detach-wait granularity
                return Result(requeue_after=self.config.detach_invisible_wait)

            t0 = time.monotonic()
            try:
                self.adapter.provider.remove_resource(resource)
            except WaitingDeviceDetaching:
                return Result(requeue_after=self._fabric_wait(resource))
            finally:
                self.metrics.fabric_request_seconds.labels(
                    self.adapter.provider.name, "remove"
                ).observe(time.monotonic() - t0)

            if mode == "DEVICE_PLUGIN":
                # fatal on detach (composableresource_controller.go:379-385)
                self._restart_plugin_daemonsets(resource, fatal=True)
            ops.refresh_after_detach(node)

            if mode == "DRA":
                visible = ops.is_visible_dra(node, resource.status.device_id)
            else:
                visible = ops.is_visible(node, resource.status.device_id)
            if visible:
                return Result(requeue_after=self.config.detach_invisible_wait)

            ops.remove_cdi(node, resource.status.device_id)

            if mode == "DRA":
                taints.delete_device_taint(self.client, resource)

            self._fabric_polls.pop(resource.metadata.uid, None)
            resource.status.error = ""
            resource.status.device_id = ""
            resource.status.cdi_device_id = ""
            resource.status.fabric_wait_started = ""  # wait concluded
            resource = self.client.update_status(resource)
            self._scrub_done.pop(resource.metadata.uid, None)
            started = self._detach_started.pop(resource.metadata.uid, None)
            if started is not None:
                self.metrics.detach_seconds.observe(time.monotonic() - started)
            self.recorder.normal(resource, "Detached", "device returned to fabric pool")

        resource.status.state = "Deleting"
        self.client.update_status(resource)
        return Result()

    def _handle_deleting(self, resource: ComposableResource) -> Result:
        if FINALIZER in resource.metadata.finalizers:
            resource.metadata.finalizers.remove(FINALIZER)
        self.client.update(resource)
        return Result()
