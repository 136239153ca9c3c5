// SyncServer#syncAsync / #exportUser / #isHandedOver (js/evolu_evm.js) on cases
// prepared by tests/test_gpu_napi_async.py.  Prints one JSON object:
//   same:    syncAsync over `calls`, awaited call by call
//   order:   the calls of `order` issued without awaiting, then awaited together
//   pendingThrows: close() while those calls are pending throws
//   settledEarly / blockingSettledEarly: after a dozen microtask turns, is the
//            Promise of syncAsync settled?  and that of a blocking sync()
//            wrapped in an async function (the control: it is)
//   safety:  per call of `safety.calls` the answers; `exports` holds, for every
//            user first answered null, exportUser(user) taken right after that call
//   handed:  isHandedOver of `safety.ask`
//   overlap: two calls issued without awaiting, the first answering null for
//            `overlap.user`; from the first call's continuation, with the
//            second still pending, exportUser / isHandedOver / handOver /
//            logInfo work (at once, and again a few microtask turns later,
//            when the second call's round is in flight), and close(), save(),
//            compact(), sync() and Engine#close() throw
// An answer is the response (base64), 500, or null.
"use strict";
const fs = require("fs");
const { Engine, SyncServer } = require("./evolu_evm.js");

const cases = JSON.parse(fs.readFileSync(process.argv[2], "utf8"));
const bin = (call) => call.map((b) => Buffer.from(b, "base64"));
const enc = (res) => res.map((r) => (r === null || r === 500 ? r : Buffer.from(r).toString("base64")));

async function main() {
  const eng = new Engine(0);
  const out = {};
  // ---- the same answers as sync
  let srv = new SyncServer(eng, cases.users);
  out.same = [];
  for (const call of cases.calls) out.same.push(...enc(await srv.syncAsync(bin(call))));
  srv.close();
  // ---- issue order without awaiting
  srv = new SyncServer(eng, cases.users);
  const ps = cases.order.map((call) => srv.syncAsync(bin(call)));
  out.pendingThrows = false;
  try {
    srv.close();
  } catch (e) {
    out.pendingThrows = /pending/.test(e.message);
  }
  out.order = (await Promise.all(ps)).map(enc);
  // ---- really asynchronous: no clock, only microtask turns
  const probe = async (p) => {
    let settled = false;
    p.then(() => { settled = true; }, () => { settled = true; });
    for (let k = 0; k < 12; k++) await Promise.resolve();
    const early = settled;
    await p;
    return early;
  };
  const body = bin(cases.order[0]);
  out.settledEarly = await probe(srv.syncAsync(body));
  out.blockingSettledEarly = await probe((async () => srv.sync(body))());
  srv.close();
  // ---- state safety
  srv = new SyncServer(eng, cases.users);
  out.safety = [];
  out.exports = {};
  for (let c = 0; c < cases.safety.calls.length; c++) {
    const res = await srv.syncAsync(bin(cases.safety.calls[c]));
    out.safety.push(enc(res));
    res.forEach((r, i) => {
      const u = cases.safety.users[c][i];
      if (r === null && !(u in out.exports)) {
        const e = srv.exportUser(u);
        out.exports[u] = e === null ? null : Buffer.from(e).toString("base64");
      }
    });
  }
  out.handed = {};
  for (const u of cases.safety.ask) out.handed[u] = srv.isHandedOver(u);
  out.exportUnknown = srv.exportUser("nobody-by-that-name");
  srv.close();
  // ---- INTEGRATION.md's handler with overlapping batches
  srv = new SyncServer(eng, cases.users);
  const ov = cases.overlap;
  await srv.syncAsync(bin(ov.setup));
  const o = out.overlap = { secondSettledAtExport: [], exports: [], handed: [], throws: {} };
  let secondSettled = false;
  const p1 = srv.syncAsync(bin(ov.first));
  const p2 = srv.syncAsync(bin(ov.second));
  p2.then(() => { secondSettled = true; }, () => { secondSettled = true; });
  const b64 = (e) => (e === null ? null : Buffer.from(e).toString("base64"));
  const first = p1.then(async (res) => {
    o.first = enc(res);
    for (let turn = 0; turn < 2; turn++) {
      o.secondSettledAtExport.push(secondSettled);
      o.exports.push(b64(srv.exportUser(ov.user)));
      o.handed.push(srv.isHandedOver(ov.user));
      o.rows = srv.logInfo().rows;
      for (let k = 0; k < 6; k++) await Promise.resolve();  // (the second call's round is queued by now)
    }
    srv.handOver(ov.user);  // (already handed over: no change)
    const tries = { close: () => srv.close(), save: () => srv.save(ov.path), compact: () => srv.compact(),
      sync: () => srv.sync(bin(ov.second)), engineClose: () => eng.close() };
    for (const name of Object.keys(tries)) {
      try {
        tries[name]();
        o.throws[name] = false;
      } catch (e) {
        o.throws[name] = /pending/.test(e.message);
      }
    }
  });
  await first;
  o.second = enc(await p2);
  o.exportAfter = b64(srv.exportUser(ov.user));
  srv.close();
  eng.close();
  console.log(JSON.stringify(out));
}

main().catch((e) => {
  console.error(e);
  process.exit(1);
});
