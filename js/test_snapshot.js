// Runs SyncServer over bodies prepared by tests/test_gpu_napi_snapshot.py:
// the calls before the restart, compact + save, a fresh SyncServer.load, the
// calls after it.  Prints per body the response (base64), 500 or null, and
// the log's shape at each step, as JSON.
"use strict";
const fs = require("fs");
const { Engine, SyncServer } = require("./evolu_evm.js");

const cases = JSON.parse(fs.readFileSync(process.argv[2], "utf8"));
const eng = new Engine(0);
const out = { answers: [], log: {} };
const run = (srv, calls) => {
  for (const call of calls) {
    const res = srv.sync(call.map((b) => Buffer.from(b, "base64")));
    res.forEach((r) => out.answers.push(r === null || r === 500 ? r : Buffer.from(r).toString("base64")));
  }
};
let srv = new SyncServer(eng, cases.users);
run(srv, cases.before);
out.log.before = srv.logInfo();
srv.compact();
out.log.compacted = srv.logInfo();
srv.save(cases.path);
out.log.saved = srv.logInfo();
srv.close();
srv = SyncServer.load(eng, cases.path, cases.usersAfter);
out.log.loaded = srv.logInfo();
run(srv, cases.after);
srv.close();
// a damaged file: nothing loaded, the status reaches the caller
const bad = Buffer.from(fs.readFileSync(cases.path));
bad[bad.length >> 1] ^= 0x10;
fs.writeFileSync(cases.path + ".bad", bad);
try {
  SyncServer.load(eng, cases.path + ".bad", cases.usersAfter);
  out.damaged = "loaded";
} catch (e) {
  out.damaged = e.code;  // (the status, as a string)
}
eng.close();
console.log(JSON.stringify(out));
